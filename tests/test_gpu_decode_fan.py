"""Fan-out decoding on the MI355X (n continuations of one cached prompt): the decode_*_fan kernels bit for bit against the single-position
kernels on the replicated history, one case at 2^20 positions that is also held to the sliced fp64 direct sum, HyenaDNALM teacher forcing
against every row's own full forward (fp32 and bf16 autocast), and the graphed fan-out step against the eager one with the device sampler."""
import pytest
import torch

from tests.test_decode_fan_emu import FanCase, direct_sum_check

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fan_kernels_equal_single_position_kernels_on_replicated_history(gpu_lib, dtype):
    c = FanCase(gpu_lib, D=256, G=2, n=3, Lcap=3 * 8192 + 64, P=2 * 8192 + 5, dtype=dtype, dev=DEV, seed=1)
    assert c.S == 2 * 8192
    c.assert_steps_bitwise(gpu_lib, 3)


def test_fan_kernels_long_history(gpu_lib):
    """2^20 positions: 127 shared chunks and one of the rows' own; bitwise against the replicated single-position kernels, and one row
    against the fp64 direct sum"""
    L = 1 << 20
    c = FanCase(gpu_lib, D=8, G=1, n=4, Lcap=L, P=L - 64, dtype=torch.bfloat16, dev=DEV, seed=2)
    assert c.S == L - 8192
    x2, tail_in = c.new_x2(), c.tail_fan.clone()
    z1, g1 = c.step_one(gpu_lib, x2)
    z2, g2 = c.step_fan(gpu_lib, x2)
    assert torch.equal(z1, z2) and torch.equal(g1, g2) and torch.equal(c.tail_one, c.tail_fan) and not torch.isnan(z2.float()).any()
    assert torch.equal(c.full[:, :, c.P], c.rows[:, :, c.P - c.S]) and c.pos_fan.item() == c.P + 1 and c.pos_one.item() == c.P + 1
    direct_sum_check(c, z2, g2, x2, tail_in, 2, c.P)


def _lm(L, d, n_layer, seed=0):
    from hyena_dna_amd.lm import HyenaDNALM
    torch.manual_seed(seed)
    layer = dict(l_max=L + 2, order=2, filter_order=64, emb_dim=5, short_filter_order=3, modulate=True, w=10, lr=6e-4, wd=0.0, lr_pos_emb=0.0)
    return HyenaDNALM(d_model=d, n_layer=n_layer, d_inner=4 * d, vocab_size=12, layer=layer, resid_dropout=0.0, embed_dropout=0.1,
                      pad_vocab_size_multiple=8, fused_dropout_add_ln=True, residual_in_fp32=True).to(DEV).eval()


@pytest.mark.parametrize("autocast", [False, True])
def test_lm_fan_cached_logits_match_each_rows_full_forward(gpu_lib, autocast):
    """teacher forcing: G = 2 prompts of 8200 tokens, n = 2 rows each with their own 8 next tokens; every row's logits at positions
    P - 1 ... P + 7 against one plain forward over that row's own P + 8 tokens"""
    from hyena_dna_amd.inference import InferenceParams
    G, n, P, N, d, n_layer = 2, 2, 8200, 8, 128, 2
    B = G * n
    m = _lm(P + N, d, n_layer)
    gen = torch.Generator().manual_seed(P)
    prompts = torch.randint(7, 11, (G, P), generator=gen).to(DEV)
    cont = torch.stack([torch.randperm(4, generator=gen) + 7 for _ in range(N)], dim=1).to(DEV)      # distinct tokens per row at every step
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        ip = InferenceParams(max_seqlen=P + N, max_batch_size=B)
        ip.key_value_memory_dict = m.allocate_inference_cache(B, P + N, fan=n, prompt_len=P)
        assert all(st.S == 8192 and st.hist_shared.shape[0] == G for st in ip.key_value_memory_dict.values())
        outs = [m(prompts, inference_params=ip)[0].logits[:, -1:].float().repeat_interleave(n, 0)]
        for i in range(N):
            ip.seqlen_offset = P + i
            outs.append(m(cont[:, i:i + 1], inference_params=ip)[0].logits.float())
        got = torch.cat(outs, dim=1)                                                                  # (B, N + 1, V)
        tol = 1e-5 if not autocast else 2e-2
        for r in range(B):
            ref = m(torch.cat([prompts[r // n], cont[r]])[None])[0].logits[0, P - 1:P + N].float()
            assert ref.shape == got[r].shape
            assert _rel(got[r], ref) < tol, (r, _rel(got[r], ref))
            for i in range(N + 1):
                assert _rel(got[r, i], ref[i]) < (tol if not autocast else 3e-2), (r, i, _rel(got[r, i], ref[i]))


def test_graphed_fan_step_is_bitwise_the_eager_step(gpu_lib):
    import hyena_dna_amd
    assert hyena_dna_amd.GRAPH_SAFE
    G, n, P, N = 2, 4, 8200, 12
    m = _lm(P + N, 128, 2)
    ids = torch.randint(7, 11, (G, P), generator=torch.Generator().manual_seed(G)).to(DEV)
    runs = []
    for cg in (False, True, True):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = m.generate(ids, max_length=P + N, use_cache=True, cg=cg, num_return_sequences=n, sampler="device", seed=11, top_k=4,
                             return_dict_in_generate=True, output_scores=True)
        runs.append((out.sequences, torch.stack(out.scores)))
    (s0, l0), (s1, l1), (s2, l2) = runs
    assert s0.shape == (G * n, P + N) and l0.shape[:2] == (N, G * n)
    assert torch.equal(s0, s1) and torch.equal(l0, l1)                # replay == eager step, bit for bit
    assert torch.equal(s1, s2) and torch.equal(l1, l2)                # and two graphed runs agree
    assert torch.equal(s0[:, :P], ids.repeat_interleave(n, 0)) and (s0[:, P:] < 16).all()
    for g in range(G):                                                # the draw depends on the row
        assert not all(torch.equal(s0[g * n], s0[g * n + j]) for j in range(1, n)), g
