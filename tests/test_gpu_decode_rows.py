"""Cached generation for prompts of different lengths on the MI355X: the per-row decode kernels against an fp64 direct sum up to 2^20
positions, uniform positions against the single-position kernels bit for bit, HyenaDNALM's per-row cached logits against a full forward of
every row's own unpadded sequence (fp32 and bf16 autocast), the graphed ragged step against the eager one (bitwise) and run to run."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _inputs(_lib, D, B, Lcap, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    lda = _lib.row_pitch(Lcap)
    k = torch.randn(D, lda, generator=g, device=DEV) * torch.exp(-3.0 * torch.linspace(0, 1, lda, device=DEV))[None]
    return dict(k=k[:, :Lcap], lda=lda, fb=torch.randn(D, generator=g, device=DEV), w=torch.randn(3 * D, 3, generator=g, device=DEV) * 0.5,
                b=torch.randn(3 * D, generator=g, device=DEV) * 0.2, bin=torch.randn(3 * D, generator=g, device=DEV) * 0.3,
                hist=torch.randn(B, D, lda, generator=g, device=DEV).to(dtype),
                tail=torch.randn(3 * D, B, 2, generator=g, device=DEV).to(dtype).float(),
                x2=torch.randn(B, 3 * D, generator=g, device=DEV).to(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Lcap,ts,D", [(4096, (0, 63, 4095), 256), (1 << 20, (64, (1 << 19) + 5), 8)])
def test_rows_kernels_vs_direct_sum(gpu_lib, dtype, Lcap, ts, D):
    _lib = gpu_lib
    B = len(ts)
    a = _inputs(_lib, D, B, Lcap, dtype, Lcap)
    hist, tail = a["hist"], a["tail"].clone()
    pos = torch.tensor(ts, dtype=torch.int32, device=DEV)
    x0 = torch.empty(B, D, device=DEV)
    z = torch.empty(B, D, dtype=dtype, device=DEV)
    part = _lib.decode_partials(B, D, Lcap, DEV).fill_(float("nan"))         # a slot that was not written in this step must never be read
    _lib.decode_pre_rows(a["x2"], a["bin"], a["w"], a["b"], tail, hist, x0, pos, Lcap)
    _lib.decode_conv_rows(a["k"], hist, part, pos, B, Lcap)
    _lib.decode_post_rows(part, hist, a["fb"], x0, z, pos, B, Lcap)
    assert pos.tolist() == [t + 1 for t in ts]
    tol = 1e-5 if dtype == torch.float32 else 2 ** -7
    for r, t in enumerate(ts):
        c = []
        for sl in (slice(0, D), slice(D, 2 * D), slice(2 * D, 3 * D)):
            xm2, xm1, xn = a["tail"][sl, r, 0].double(), a["tail"][sl, r, 1].double(), a["x2"][r, sl].double()
            bi, ww = a["bin"][sl].double(), a["w"][sl].double()
            x0v = xm2 + bi if t >= 2 else torch.zeros_like(xn)
            x1v = xm1 + bi if t >= 1 else torch.zeros_like(xn)
            c.append(a["b"][sl].double() + ww[:, 0] * x0v + ww[:, 1] * x1v + ww[:, 2] * (xn + bi))
        assert _rel(hist[r, :, t], c[1] * c[2]) < tol
        assert torch.equal(tail[:, r, 0], a["tail"][:, r, 1]) and torch.equal(tail[:, r, 1], a["x2"][r].float())
        y = torch.zeros(D, dtype=torch.float64, device=DEV)
        for s0 in range(0, t + 1, 1 << 16):                      # fp64 direct sum in slices (memory)
            s1 = min(t + 1, s0 + (1 << 16))
            y += (hist[r, :, s0:s1].double() * a["k"][:, t - s1 + 1:t - s0 + 1].double().flip(-1)).sum(-1)
        y += a["fb"].double() * hist[r, :, t].double()
        zr = y.to(dtype).double() * c[0]
        if dtype == torch.float32:
            assert _rel(z[r], zr) < 1e-5, (r, t, _rel(z[r], zr))
        else:
            err = (z[r].double() - zr).abs()
            assert (err <= tol * zr.abs() + 1e-6 + 2 * tol * y.abs() * c[0].abs()).all(), (r, t, err.max().item())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rows_uniform_positions_equal_single_position_kernels(gpu_lib, dtype):
    _lib = gpu_lib
    D, B, Lcap = 256, 3, 4096
    a = _inputs(_lib, D, B, Lcap, dtype, 11)
    for t in (0, 64, 4095):
        got = []
        for rows in (True, False):
            hist, tail = a["hist"].clone(), a["tail"].clone()
            pos = torch.full((B if rows else 1,), t, dtype=torch.int32, device=DEV)
            x0, z, part = torch.empty(B, D, device=DEV), torch.empty(B, D, dtype=dtype, device=DEV), _lib.decode_partials(B, D, Lcap, DEV)
            part.zero_()
            pre, conv, post = ((_lib.decode_pre_rows, _lib.decode_conv_rows, _lib.decode_post_rows) if rows else
                               (_lib.decode_pre, _lib.decode_conv, _lib.decode_post))
            pre(a["x2"], a["bin"], a["w"], a["b"], tail, hist, x0, pos, Lcap)
            conv(a["k"], hist, part, pos, B, Lcap)
            post(part, hist, a["fb"], x0, z, pos, B, Lcap)
            assert pos.tolist() == [t + 1] * pos.numel()
            got.append((z, hist, tail, x0, part))
        for x, y in zip(*got):
            assert torch.equal(x, y), t


def _lm(L, d, n_layer, seed=0):
    from hyena_dna_amd.lm import HyenaDNALM
    torch.manual_seed(seed)
    layer = dict(l_max=L + 2, order=2, filter_order=64, emb_dim=5, short_filter_order=3, modulate=True, w=10, lr=6e-4, wd=0.0, lr_pos_emb=0.0)
    return HyenaDNALM(d_model=d, n_layer=n_layer, d_inner=4 * d, vocab_size=12, layer=layer, resid_dropout=0.0, embed_dropout=0.1,
                      pad_vocab_size_multiple=8, fused_dropout_add_ln=True, residual_in_fp32=True).to(DEV).eval()


@pytest.mark.parametrize("autocast", [False, True])
def test_lm_ragged_cached_logits_match_each_rows_full_forward(gpu_lib, autocast):
    """teacher forcing: row b's logits at positions lengths[b] - 1 ... lengths[b] + 7 from one right-padded prefill and 8 per-row steps,
    against one plain forward over row b's own lengths[b] + 8 tokens"""
    from hyena_dna_amd.inference import InferenceParams
    L, d, n_layer, N = 1024, 128, 2, 8
    lens = (1000, 513, 64, 1)
    B, P = len(lens), max(lens)
    m = _lm(L, d, n_layer)
    full = torch.randint(7, 11, (B, P + N), generator=torch.Generator().manual_seed(L + B)).to(DEV)      # row b: its first lens[b] + N tokens
    lengths = torch.tensor(lens, dtype=torch.int32, device=DEV)
    cols = torch.arange(P, device=DEV)
    prompt = torch.where(cols[None] < lengths[:, None], full[:, :P], torch.full_like(full[:, :P], 9))       # right-padded with a valid token
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        ip = InferenceParams(max_seqlen=P + N, max_batch_size=B, lengths_per_sample=lengths)
        ip.key_value_memory_dict = m.allocate_inference_cache(B, P + N)
        logits = m(prompt, inference_params=ip)[0].logits
        outs = [logits.gather(1, (lengths.long() - 1)[:, None, None].expand(B, 1, logits.shape[-1])).float()]
        for i in range(N):
            ip.seqlen_offset = P + i
            tok = full.gather(1, (lengths.long() + i)[:, None])
            outs.append(m(tok, inference_params=ip)[0].logits.float())
        got = torch.cat(outs, dim=1)                                                                        # (B, N + 1, V)
        tol = 1e-5 if not autocast else 2e-2
        for r, n in enumerate(lens):
            ref = m(full[r:r + 1, :n + N])[0].logits[0, n - 1:n + N].float()
            assert ref.shape == got[r].shape
            assert _rel(got[r], ref) < tol, (r, _rel(got[r], ref))
            for i in range(N + 1):
                assert _rel(got[r, i], ref[i]) < (tol if not autocast else 3e-2), (r, i, _rel(got[r, i], ref[i]))


def test_graphed_ragged_step_is_bitwise_the_eager_step(gpu_lib):
    import hyena_dna_amd
    assert hyena_dna_amd.GRAPH_SAFE
    m = _lm(1024, 128, 2)
    lens = (900, 517, 64, 3)
    B, P, N = len(lens), max(lens), 6
    ids = torch.randint(7, 11, (B, P), generator=torch.Generator().manual_seed(B)).to(DEV)
    lengths = torch.tensor(lens, dtype=torch.int32, device=DEV)
    runs = []
    for cg in (False, True, False):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = m.generate(ids, max_length=P + N, use_cache=True, cg=cg, lengths=lengths, pad_token_id=4, return_dict_in_generate=True,
                             output_scores=True)
        runs.append((out.sequences, torch.stack(out.scores)))
        assert out.lengths.tolist() == [n + N for n in lens]
    (s0, l0), (s1, l1), (s2, l2) = runs
    assert torch.equal(s0, s1) and torch.equal(l0, l1)                # replay == eager step, bit for bit
    assert torch.equal(s0, s2) and torch.equal(l0, l2)                # and two identical eager runs agree
    for r, n in enumerate(lens):
        assert torch.equal(s0[r, :n], ids[r, :n]) and (s0[r, n + N:] == 4).all() and (s0[r, n:n + N] < 16).all()
