"""The block decode step on the MI355X: the decode_*_block kernels bit for bit against T calls of the single-position kernels (plain and
fan-out layout, three dtypes; one case at d = 256 with four rows), HyenaDNALM's appended logits against the full forward (fp32 and bf16
autocast, the tolerances of tests/test_gpu_decode.py), score_continuations against one full forward per candidate, and run-to-run equality."""
import pytest
import torch

from tests.test_decode_block_emu import DTYPES, FAN_CASES, PLAIN_CASES, BlockCase

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Lcap,t0,T", PLAIN_CASES)
def test_block_kernels_equal_single_steps(gpu_lib, dtype, Lcap, t0, T):
    c = BlockCase(gpu_lib, D=5, G=2, n=1, Lcap=Lcap, t0=t0, dtype=dtype, dev=DEV, seed=Lcap + t0 + T)
    c.assert_block_bitwise(T)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Lcap,P,t0,T", FAN_CASES)
def test_block_fan_kernels_equal_single_fan_steps(gpu_lib, dtype, Lcap, P, t0, T):
    c = BlockCase(gpu_lib, D=5, G=2, n=3, Lcap=Lcap, t0=t0, dtype=dtype, fan=True, P=P, dev=DEV, seed=Lcap + P + t0 + T)
    c.assert_block_bitwise(T)


@pytest.mark.parametrize("fan", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_block_kernels_d256(gpu_lib, dtype, fan):
    c = BlockCase(gpu_lib, D=256, G=4 if not fan else 2, n=1 if not fan else 2, Lcap=16500, t0=16389, dtype=dtype, fan=fan, P=16389, dev=DEV, seed=4)
    assert c.B == 4
    c.assert_block_bitwise(64)


@pytest.mark.parametrize("fan", [False, True])
def test_block_out_of_range_does_nothing(gpu_lib, fan):
    c = BlockCase(gpu_lib, D=5, G=2, n=3 if fan else 1, Lcap=8300, t0=8290, dtype=torch.bfloat16, fan=fan, P=8200, dev=DEV, seed=3)
    rows, tail = c.blk["rows"].clone(), c.blk["tail"].clone()
    z, x0 = c.step_block(c.new_x(11))                                            # t0 + T = Lcap + 1
    assert torch.isnan(z.float()).all() and torch.isnan(x0).all()
    assert torch.equal(c.blk["rows"], rows) and torch.equal(c.blk["tail"], tail) and c.blk["pos"].item() == 8290
    c.assert_block_bitwise(10)


def test_two_block_runs_are_equal(gpu_lib):
    outs = []
    for _ in range(2):
        c = BlockCase(gpu_lib, D=64, G=2, n=2, Lcap=16500, t0=16389, dtype=torch.bfloat16, fan=True, P=8200, dev=DEV, seed=6)
        z, x0 = c.step_block(c.new_x(64))
        outs.append((z, x0, c.blk["rows"], c.blk["tail"], c.blk["pos"]))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def _lm(L, d, n_layer, seed=0):
    from hyena_dna_amd.lm import HyenaDNALM
    torch.manual_seed(seed)
    layer = dict(l_max=L + 2, order=2, filter_order=64, emb_dim=5, short_filter_order=3, modulate=True, w=10, lr=6e-4, wd=0.0, lr_pos_emb=0.0)
    return HyenaDNALM(d_model=d, n_layer=n_layer, d_inner=4 * d, vocab_size=12, layer=layer, resid_dropout=0.0, embed_dropout=0.1,
                      pad_vocab_size_multiple=8, fused_dropout_add_ln=True, residual_in_fp32=True).to(DEV).eval()


def _assert_logits(got, ref, autocast, what):
    """tests/test_gpu_decode.py's bounds: 1e-5 in fp32; under bf16 autocast 2e-2 over a row's positions and 3e-2 per position"""
    figures = [(r, _rel(got[r], ref[r]), max(_rel(got[r, i], ref[r, i]) for i in range(ref.shape[1]))) for r in range(ref.shape[0])]
    print(what, "autocast" if autocast else "fp32", [(r, f"{a:.2e}", f"{p:.2e}") for r, a, p in figures])
    for r, overall, worst in figures:
        assert overall < (2e-2 if autocast else 1e-5), (what, r, overall)
        assert worst < (3e-2 if autocast else 1e-5), (what, r, worst)


@pytest.mark.parametrize("autocast", [False, True])
@pytest.mark.parametrize("L,d,P,T,B", [(1024, 128, 960, 63, 1), (1024, 128, 960, 63, 4), (32768, 256, 16380, 40, 1)])
def test_lm_appended_block_matches_full_forward(gpu_lib, autocast, L, d, P, T, B):
    from hyena_dna_amd.inference import InferenceParams
    m = _lm(L, d, 2)
    ids = torch.randint(7, 11, (B, P + T), generator=torch.Generator().manual_seed(P)).to(DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        ref = m(ids)[0].logits[:, P:].float()
        ip = InferenceParams(max_seqlen=L, max_batch_size=B, allow_append=True)
        ip.key_value_memory_dict = m.allocate_inference_cache(B, L)
        m(ids[:, :P], inference_params=ip)
        ip.seqlen_offset = P
        got = m(ids[:, P:], inference_params=ip)[0].logits.float()
    assert got.shape == ref.shape and all(st.pos.item() == P + T for st in ip.key_value_memory_dict.values())
    _assert_logits(got, ref, autocast, f"block {L}x{d} P={P} T={T} B={B}")


def test_score_continuations_matches_full_forwards(gpu_lib):
    L, d, P, n, T = 32768, 256, 16389, 4, 33
    m = _lm(L, d, 2)
    gen = torch.Generator().manual_seed(8)
    ctx = torch.randint(7, 11, (1, P), generator=gen).to(DEV)
    cont = torch.randint(7, 11, (1, n, T), generator=gen).to(DEV)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        lp, logits = m.score_continuations(ctx, cont, vocab_size=12, return_logits=True)
        with torch.no_grad():
            ref = torch.cat([m(torch.cat([ctx[0], cont[0, j]])[None])[0].logits[:, P - 1:P + T - 1].float() for j in range(n)])
    assert lp.shape == (1, n, T) and logits.shape == (1, n, T, 16)
    assert torch.equal(lp, torch.log_softmax(logits[..., :12], dim=-1).gather(-1, cont.unsqueeze(-1)).squeeze(-1))
    _assert_logits(logits[0], ref, True, "score_continuations")
