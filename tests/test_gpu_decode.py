"""Incremental decoding on the MI355X: the decode kernels against an fp64 direct sum at D = 256 up to 2^20 positions, HyenaDNALM prefill + 64
steps against one full forward (fp32 and bf16 autocast, B = 1 and 4, up to a 2^20-position context), the graphed step against the eager one
(bitwise) and run-to-run determinism."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Lcap,ts,B", [(4096, (0, 63, 64, 4095), 3), (1 << 20, (0, 64, (1 << 19) + 5, (1 << 20) - 1), 1)])
def test_decode_kernels_vs_direct_sum(gpu_lib, dtype, Lcap, ts, B):
    _lib = gpu_lib
    D = 256
    g = torch.Generator(device=DEV).manual_seed(Lcap)
    lda = _lib.row_pitch(Lcap)
    k = torch.randn(D, lda, generator=g, device=DEV) * torch.exp(-3.0 * torch.linspace(0, 1, lda, device=DEV))[None]
    k = k[:, :Lcap]
    fb = torch.randn(D, generator=g, device=DEV)
    w = torch.randn(3 * D, 3, generator=g, device=DEV) * 0.5
    b = torch.randn(3 * D, generator=g, device=DEV) * 0.2
    bin_ = torch.randn(3 * D, generator=g, device=DEV) * 0.3
    hist = torch.randn(B, D, lda, generator=g, device=DEV).to(dtype)
    part = _lib.decode_partials(B, D, Lcap, DEV)
    for t in ts:
        tail = torch.randn(3 * D, B, 2, generator=g, device=DEV).to(dtype).float()
        x2 = torch.randn(B, 3 * D, generator=g, device=DEV).to(dtype)
        pos = torch.tensor([t], dtype=torch.int32, device=DEV)
        x0 = torch.empty(B, D, device=DEV)
        z = torch.empty(B, D, dtype=dtype, device=DEV)
        tail_in = tail.clone()
        _lib.decode_pre(x2, bin_, w, b, tail, hist, x0, pos, Lcap)
        _lib.decode_conv(k, hist, part, pos, B, Lcap)
        _lib.decode_post(part, hist, fb, x0, z, pos, B, Lcap)
        assert pos.item() == t + 1
        c = []
        for sl in (slice(0, D), slice(D, 2 * D), slice(2 * D, 3 * D)):
            xm2, xm1, xn = tail_in[sl, :, 0].double(), tail_in[sl, :, 1].double(), x2[:, sl].double().T
            bi, ww = bin_[sl].double()[:, None], w[sl].double()
            x0v = xm2 + bi if t >= 2 else torch.zeros_like(xn)
            x1v = xm1 + bi if t >= 1 else torch.zeros_like(xn)
            c.append(b[sl].double()[:, None] + ww[:, 0:1] * x0v + ww[:, 1:2] * x1v + ww[:, 2:3] * (xn + bi))
        tol = 1e-5 if dtype == torch.float32 else 2 ** -7
        assert _rel(hist[:, :, t], (c[1] * c[2]).T) < tol
        y = torch.zeros(B, D, dtype=torch.float64, device=DEV)
        for s0 in range(0, t + 1, 1 << 16):                      # fp64 direct sum in slices (memory)
            s1 = min(t + 1, s0 + (1 << 16))
            y += (hist[:, :, s0:s1].double() * k[:, t - s1 + 1:t - s0 + 1].double().flip(-1)[None]).sum(-1)
        y += fb.double()[None] * hist[:, :, t].double()
        zr = y.to(dtype).double() * c[0].T
        if dtype == torch.float32:
            assert _rel(z, zr) < 1e-5, (t, _rel(z, zr))
        else:
            err = (z.double() - zr).abs()
            assert (err <= tol * zr.abs() + 1e-6 + 2 * tol * y.abs() * c[0].T.abs()).all(), (t, err.max().item())


def _lm(L, d, n_layer, seed=0):
    from hyena_dna_amd.lm import HyenaDNALM
    torch.manual_seed(seed)
    layer = dict(l_max=L + 2, order=2, filter_order=64, emb_dim=5, short_filter_order=3, modulate=True, w=10, lr=6e-4, wd=0.0, lr_pos_emb=0.0)
    return HyenaDNALM(d_model=d, n_layer=n_layer, d_inner=4 * d, vocab_size=12, layer=layer, resid_dropout=0.0, embed_dropout=0.1,
                      pad_vocab_size_multiple=8, fused_dropout_add_ln=True, residual_in_fp32=True).to(DEV).eval()


def _cached_logits(m, ids, P, autocast):
    from hyena_dna_amd.inference import InferenceParams
    B, L = ids.shape
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        ip = InferenceParams(max_seqlen=L, max_batch_size=B)
        ip.key_value_memory_dict = m.allocate_inference_cache(B, L)
        outs = [m(ids[:, :P], inference_params=ip)[0].logits[:, -1:].float()]
        for i in range(P, L - 1):
            ip.seqlen_offset = i
            outs.append(m(ids[:, i:i + 1], inference_params=ip)[0].logits.float())
        del ip
    return torch.cat(outs, dim=1)                                                  # positions P - 1 ... L - 2


@pytest.mark.parametrize("L,d,n_layer", [(1024, 128, 2), (32768, 256, 8)])
@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("autocast", [False, True])
def test_lm_cached_logits_match_full_forward(gpu_lib, L, d, n_layer, B, autocast):
    m = _lm(L, d, n_layer)
    ids = torch.randint(7, 11, (B, L + 1), generator=torch.Generator().manual_seed(L + B)).to(DEV)[:, :L]
    P = L - 64
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        ref = m(ids)[0].logits[:, P - 1:L - 1].float()
    got = _cached_logits(m, ids, P, autocast)
    tol = 1e-5 if not autocast else 2e-2
    assert got.shape == ref.shape
    assert _rel(got, ref) < tol, _rel(got, ref)
    for i in range(ref.shape[1]):
        assert _rel(got[:, i], ref[:, i]) < (tol if not autocast else 3e-2), (i, _rel(got[:, i], ref[:, i]))


def test_lm_cached_logits_long_context(gpu_lib):
    """one case at 2^20: d_model 256, 8 layers, a 2^20 - 64 prompt and 64 steps against a single full forward (bf16 autocast)"""
    L = 1 << 20
    m = _lm(L, 256, 8)
    ids = torch.randint(7, 11, (1, L), generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        ref = m(ids)[0].logits[:, L - 65:L - 1].float()
    torch.cuda.empty_cache()
    got = _cached_logits(m, ids, L - 64, True)
    assert _rel(got, ref) < 2e-2, _rel(got, ref)


@pytest.mark.parametrize("B", [1, 4])
def test_graphed_step_is_bitwise_the_eager_step(gpu_lib, B):
    import hyena_dna_amd
    assert hyena_dna_amd.GRAPH_SAFE
    m = _lm(1024, 128, 2)
    ids = torch.randint(7, 11, (B, 900), generator=torch.Generator().manual_seed(B)).to(DEV)
    runs = []
    for cg in (False, True, False):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = m.generate(ids, max_length=964, use_cache=True, cg=cg, return_dict_in_generate=True, output_scores=True)
        runs.append((out.sequences, torch.stack(out.scores)))
    (s0, l0), (s1, l1), (s2, l2) = runs
    assert torch.equal(s0, s1) and torch.equal(l0, l1)                # replay == eager step, bit for bit
    assert torch.equal(s0, s2) and torch.equal(l0, l2)                # and two identical eager runs agree


def test_cached_generation_is_deterministic(gpu_lib):
    m = _lm(32768, 256, 8)
    ids = torch.randint(7, 11, (2, 32700), generator=torch.Generator().manual_seed(3)).to(DEV)
    a = _cached_logits(m, torch.cat([ids, ids[:, :16]], dim=1), 32700, True)
    b = _cached_logits(m, torch.cat([ids, ids[:, :16]], dim=1), 32700, True)
    assert torch.equal(a, b)
