"""Incremental decoding (csrc/decode_kernels.h, hyena_dna_amd/inference.py) under tests/hipemu: the three step kernels against an fp64 direct
sum of the causal convolution, the filter's prefix consistency, HyenaOperator prefill + steps against one forward over the whole sequence,
HyenaDNALM cached logits and greedy generation against the recompute path, and every refusal."""
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SOURCES = [os.path.join(ROOT, "hyena_dna_amd", "csrc", "decode_kernels.h"), os.path.join(ROOT, "include", "hyena_decode.h")]


@pytest.fixture()
def decode_emu(emu_backend):
    """the emulation library of emu_backend, rebuilt if the decode kernels are newer than it (build_emu's freshness check does not list them)"""
    from tests.hipemu import build_emu
    if not os.path.exists(build_emu.OUT) or any(os.path.getmtime(f) > os.path.getmtime(build_emu.OUT) for f in NEW_SOURCES):
        build_emu.build(force=True)
        emu_backend._lib = None
    return emu_backend


def _layer(l_max, **kw):
    d = dict(l_max=l_max, order=2, filter_order=64, emb_dim=5, short_filter_order=3, modulate=True, w=10, lr=6e-4, wd=0.0, lr_pos_emb=0.0)
    d.update(kw)
    return d


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _sc64(xm2, xm1, xn, t, w, b, bin_):
    x0 = (xm2 + bin_) if t >= 2 else torch.zeros_like(xn)
    x1 = (xm1 + bin_) if t >= 1 else torch.zeros_like(xn)
    return b + w[:, 0:1] * x0 + w[:, 1:2] * x1 + w[:, 2:3] * (xn + bin_)


# ---- the kernels against the fp64 direct sum --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D,B,Lcap,ts", [(2, 1, 600, (0, 1, 2, 63, 64, 599)), (4, 3, 577, (0, 5, 300, 576)), (8, 3, 130, (0, 127, 129)),
                                         (2, 1, 8200, (8191, 8192, 8199)), (3, 2, 8193, (0, 8192))])
def test_decode_kernels_vs_direct_sum(decode_emu, dtype, D, B, Lcap, ts):
    _lib = decode_emu
    g = torch.Generator().manual_seed(D * 1000 + Lcap)
    lda = _lib.row_pitch(Lcap)
    k = torch.zeros(D, lda)[:, :Lcap]                                      # (rows pitched to 64 words, as the decode cache keeps them)
    k.copy_(torch.randn(D, Lcap, generator=g) * torch.exp(-3.0 * torch.linspace(0, 1, Lcap))[None])
    fb = torch.randn(D, generator=g)
    w = torch.randn(3 * D, 3, generator=g) * 0.5
    b = torch.randn(3 * D, generator=g) * 0.2
    bin_ = torch.randn(3 * D, generator=g) * 0.3
    for t in ts:
        hist = torch.randn(B, D, lda, generator=g).to(dtype)
        tail = torch.randn(3 * D, B, 2, generator=g).to(dtype).float()
        x2 = torch.randn(B, 3 * D, generator=g).to(dtype)
        pos = torch.tensor([t], dtype=torch.int32)
        x0 = torch.empty(B, D)
        z = torch.empty(B, D, dtype=dtype)
        part = _lib.decode_partials(B, D, Lcap, "cpu")
        tail_in, hist_in = tail.clone(), hist.clone()
        _lib.decode_pre(x2, bin_, w, b, tail, hist, x0, pos, Lcap)
        _lib.decode_conv(k, hist, part, pos, B, Lcap)
        _lib.decode_post(part, hist, fb, x0, z, pos, B, Lcap)
        assert pos.item() == t + 1
        # short conv + gate in fp64
        c = [_sc64(tail_in[sl, :, 0].double(), tail_in[sl, :, 1].double(), x2[:, sl].double().T, t, w[sl].double(), b[sl].double()[:, None],
                   bin_[sl].double()[:, None]) for sl in (slice(0, D), slice(D, 2 * D), slice(2 * D, 3 * D))]           # (D, B) each
        vg_t = (c[1] * c[2]).T                                                                                           # (B, D)
        tol = 1e-5 if dtype == torch.float32 else (2 ** -7 if dtype == torch.bfloat16 else 2 ** -10)
        assert _rel(hist[:, :, t], vg_t) < tol
        assert torch.equal(tail[:, :, 0], tail_in[:, :, 1]) and torch.equal(tail[:, :, 1], x2.float().T)
        # only column t of the history changed
        other = torch.ones(lda, dtype=torch.bool)
        other[t] = False
        assert torch.equal(hist[:, :, other], hist_in[:, :, other])
        # the causal sum over the history as the kernels see it (column t = the rounded vg_t just written)
        h = hist[:, :, :t + 1].double()
        kk = k[:, :t + 1].double().flip(-1)                                                                             # k[d, t - s]
        y = (h * kk[None]).sum(-1) + fb.double()[None] * h[:, :, t]
        zr = y.to(dtype).double() * c[0].T
        assert _rel(x0, c[0].T) < 1e-5
        if dtype == torch.float32:
            assert _rel(z, zr) < 1e-5, (t, _rel(z, zr))
        else:                                                                                                          # one rounding of the output
            err = (z.double() - zr).abs()
            assert (err <= tol * zr.abs() + 1e-6 + 2 * tol * y.abs() * c[0].T.abs()).all(), (t, err.max().item())


def test_decode_refuses_bad_arguments(decode_emu):
    L = decode_emu.lib()
    assert L.hyena_decode_partial_floats(2, 4, 8193) == 2 * 2 * 4 and L.hyena_decode_partial_floats(1, 4, (1 << 20) + 1) == 0
    assert L.hyena_decode_conv(None, 64, None, None, None, 1, 4, 64, 64, 0, None) == 1
    assert L.hyena_decode_pre(None, 12, None, None, None, None, None, None, None, 1, 1, 4, 64, 64, 0, None) == 1
    assert L.hyena_decode_post(None, None, None, None, None, None, 1, 4, 64, 64, 0, None) == 1


# ---- prefix consistency of the implicit filter -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128])
def test_filter_is_prefix_consistent(decode_emu, D):
    """the fused filter kernels (the route of every d_model the operator's fused path serves): column j of filter_dl(L) does not depend on L,
    bit for bit.  (The PyTorch route of other widths is a library GEMM over L columns, whose blocking may depend on L: rounding level.)"""
    from hyena_dna_amd.hyena import HyenaFilter
    torch.manual_seed(0)
    f = HyenaFilter(D, emb_dim=5, order=64, seq_len=700, w=10, lr=6e-4, wd=0.0, lr_pos_emb=0.0, modulate=True)
    with torch.no_grad():
        full = f.filter_dl(700)
        for L in (1, 2, 64, 333, 699):
            assert torch.equal(f.filter_dl(L), full[:, :L]), L


# ---- HyenaOperator: prefill P, then N steps == one forward over P + N ---------------------------------------------------------------------
@pytest.mark.parametrize("D,B,P,N", [(8, 2, 37, 9), (64, 1, 1, 6), (16, 3, 2, 5)])
def test_operator_prefill_and_steps_match_forward(decode_emu, D, B, P, N):
    from hyena_dna_amd.hyena import HyenaOperator
    from hyena_dna_amd.inference import InferenceParams
    torch.manual_seed(D + P)
    op = HyenaOperator(d_model=D, **_layer(P + N + 3))
    u = torch.randn(B, P + N, D)
    with torch.no_grad():
        ref = op(u)
        plain = op(u[:, :P])
        ip = InferenceParams(max_seqlen=P + N, max_batch_size=B)
        ip.key_value_memory_dict[op._decode_key()] = op.allocate_inference_cache(B, P + N)
        pre = op(u[:, :P], inference_params=ip)
        assert torch.equal(pre, plain)                                     # the prefill IS the plain forward
        outs = [pre]
        for i in range(N):
            ip.seqlen_offset = P + i
            outs.append(op(u[:, P + i:P + i + 1], inference_params=ip))
    got = torch.cat(outs, dim=1)
    assert _rel(got, ref) < 1e-5
    for i in range(P, P + N):
        assert _rel(got[:, i], ref[:, i]) < 1e-5, i


# ---- HyenaDNALM -------------------------------------------------------------------------------------------------------------------------
def _lm(L, d=64, n_layer=2, seed=0, **kw):
    from hyena_dna_amd.lm import HyenaDNALM
    torch.manual_seed(seed)
    m = HyenaDNALM(d_model=d, n_layer=n_layer, d_inner=4 * d, vocab_size=12, layer=_layer(L + 2), resid_dropout=0.0, embed_dropout=0.1,
                   pad_vocab_size_multiple=8, fused_dropout_add_ln=True, residual_in_fp32=True, **kw)
    return m.eval()


@pytest.mark.parametrize("checkpointed", [False, True])
def test_lm_cached_logits_match_full_forward(decode_emu, checkpointed):
    from hyena_dna_amd.inference import InferenceParams
    B, P, N = 2, 45, 8
    m = _lm(P + N, checkpoint_mixer=checkpointed, checkpoint_mlp=checkpointed)
    ids = torch.randint(7, 11, (B, P + N), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        ref = m(ids)[0].logits
        ip = InferenceParams(max_seqlen=P + N, max_batch_size=B)
        ip.key_value_memory_dict = m.allocate_inference_cache(B, P + N)
        assert len(ip.key_value_memory_dict) == 2
        outs = [m(ids[:, :P], inference_params=ip)[0].logits]
        for i in range(N):
            ip.seqlen_offset = P + i
            outs.append(m(ids[:, P + i:P + i + 1], inference_params=ip)[0].logits)
    got = torch.cat(outs, dim=1)
    assert got.shape == ref.shape
    for i in range(P - 1, P + N):
        assert _rel(got[:, i], ref[:, i]) < 1e-5, i


def test_lm_greedy_generate_with_cache_matches_recompute(decode_emu):
    B, P, n_new = 2, 30, 10
    m = _lm(P + n_new)
    ids = torch.randint(7, 11, (B, P), generator=torch.Generator().manual_seed(2))
    a = m.generate(ids, max_length=P + n_new, return_dict_in_generate=True, output_scores=True)
    b = m.generate(ids, max_length=P + n_new, use_cache=True, return_dict_in_generate=True, output_scores=True)
    assert a.sequences.shape == b.sequences.shape == (B, P + n_new)
    # teacher forcing: the cached run's scores at every generated position against the recompute run's, on the recompute run's tokens
    for i in range(n_new):
        assert _rel(b.scores[i], a.scores[i]) < 1e-5 or not torch.equal(a.sequences[:, :P + i], b.sequences[:, :P + i]), i
    assert torch.equal(a.sequences, b.sequences)


def test_overlay_exports_inference_params():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "overlay"))
    try:
        from flash_attn.utils.generation import GenerationMixin, InferenceParams
        ip = InferenceParams(max_seqlen=10, max_batch_size=2)
        ip.sequence_len_offset = 3
        assert ip.seqlen_offset == 3 and ip.key_value_memory_dict == {} and GenerationMixin is not None
    finally:
        sys.path.remove(os.path.join(ROOT, "overlay"))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(decode_emu):
    from hyena_dna_amd.hyena import HyenaOperator
    from hyena_dna_amd.inference import InferenceParams
    torch.manual_seed(0)
    with pytest.raises(NotImplementedError, match="order-2"):
        HyenaOperator(d_model=8, **_layer(64, order=3)).allocate_inference_cache(1, 32)
    with pytest.raises(NotImplementedError, match="causal"):
        HyenaOperator(d_model=8, **_layer(64, bidirectional=True)).allocate_inference_cache(1, 32)
    with pytest.raises(NotImplementedError, match="fused"):
        HyenaOperator(d_model=8, **_layer(64, num_heads=2)).allocate_inference_cache(1, 32)
    op = HyenaOperator(d_model=8, **_layer(64))
    with pytest.raises(ValueError, match="max_seqlen"):
        op.allocate_inference_cache(1, 65)
    big = HyenaOperator(d_model=8, **_layer((1 << 20) + 64))
    with pytest.raises(ValueError, match="max_seqlen"):
        big.allocate_inference_cache(1, (1 << 20) + 1)
    ip = InferenceParams(max_seqlen=8, max_batch_size=2)
    ip.key_value_memory_dict[op._decode_key()] = op.allocate_inference_cache(2, 8)
    u = torch.randn(3, 4, 8)
    with torch.no_grad():
        with pytest.raises(ValueError, match="does not fit"):
            op(u, inference_params=ip)
        op(u[:2], inference_params=ip)
        ip.seqlen_offset = 4
        with pytest.raises(ValueError, match="one position"):
            op(u[:2, :2], inference_params=ip)
        for i in range(4, 8):
            ip.seqlen_offset = i
            op(u[:2, :1], inference_params=ip)
        ip.seqlen_offset = 8
        with pytest.raises(ValueError, match="past"):
            op(u[:2, :1], inference_params=ip)
    ip.seqlen_offset = 0
    with pytest.raises(ValueError, match="inference only"):
        op(u[:2], inference_params=ip)
    with torch.no_grad(), pytest.raises(ValueError, match="no decode cache"):
        op(u[:2], inference_params=InferenceParams(max_seqlen=8, max_batch_size=2))
    m = _lm(40)
    with pytest.raises(ValueError, match="cg=True"):
        m.generate(torch.zeros(1, 4, dtype=torch.long), max_length=8, cg=True)
