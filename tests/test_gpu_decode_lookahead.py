"""MI355X: the lookahead carry (csrc/decode_kernels.h decode_carry / decode_conv_la / decode_post_la, HyenaDecodeState(lookahead=W),
generate(lookahead=W)).  The cases of tests/test_decode_lookahead_emu.py on the gfx950 library, against the same fp64 references and derived
bounds (tests/decode_lookahead_local.py), plus the shipped width (D = 256, three chunks of real work, run twice and compared bit for bit), the
cache at D = 128 and 256, bf16 autocast, and the graphed step against the eager one."""
import pytest
import torch

from tests import decode_lookahead_local as LA

pytestmark = pytest.mark.gpu
dtypes = pytest.mark.parametrize("dtype", LA.DTYPES, ids=LA.NAME.get)


def _dev():
    return torch.device("cuda", 0)


# ---- kernels ------------------------------------------------------------------------------------------------------------------------------------
@dtypes
@pytest.mark.parametrize("case", LA.CARRY_CASES + LA.CARRY_WIDE, ids=LA.case_id)
def test_carry(gpu_lib, case, dtype):
    _, a = LA.run_carry(gpu_lib, _dev(), dtype, *case, seed=sum(case), label="gpu")
    if case in LA.CARRY_WIDE:
        _, b = LA.run_carry(gpu_lib, _dev(), dtype, *case, seed=sum(case), label="gpu")
        assert LA.same_bits(a[:, :min(case[4], case[2] - case[3])], b[:, :min(case[4], case[2] - case[3])]), "two runs on fresh buffers differ"


@dtypes
@pytest.mark.parametrize("case", LA.STEP_CASES + LA.STEP_WIDE, ids=LA.case_id)
def test_steps_on_a_carry(gpu_lib, case, dtype):
    LA.run_steps(gpu_lib, _dev(), dtype, *case, with_fb=case[0] != 1 or case[1] != 5, seed=sum(case[:5]), label="gpu")


@dtypes
def test_step_at_the_end_of_the_cache_is_parked(gpu_lib, dtype):
    LA.run_parked_with_pre(gpu_lib, _dev(), dtype, 3, 5, 8260, 8252, 16)


@dtypes
def test_step_past_the_window_parks_all_but_pre(gpu_lib, dtype):
    LA.run_outside_window_with_pre(gpu_lib, _dev(), dtype, 3, 5, 8260, 8185, 16)


@dtypes
@pytest.mark.parametrize("case", LA.EQUAL_CASES, ids=LA.case_id)
def test_base_zero_is_the_plain_step(gpu_lib, case, dtype):
    LA.run_equals_plain(gpu_lib, _dev(), dtype, *case, seed=sum(case))


def test_bad_arguments(gpu_lib):
    LA.check_bad_arguments(gpu_lib, _dev())


# ---- HyenaDecodeState ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=LA.NAME.get)
@pytest.mark.parametrize("P", [3, 70, 8190])
@pytest.mark.parametrize("D", [128, 256])
def test_state_over_two_refreshes(gpu_lib, D, P, dtype):
    LA.run_state(_dev(), D, P, W=8, T=dtype, label="gpu")


# ---- HyenaDNALM ---------------------------------------------------------------------------------------------------------------------------------
def _lm(L, d=128, n_layer=2, seed=0):
    from hyena_dna_amd.lm import HyenaDNALM
    torch.manual_seed(seed)
    return HyenaDNALM(d_model=d, n_layer=n_layer, d_inner=4 * d, vocab_size=12, layer=LA._layer(L + 2), resid_dropout=0.0, embed_dropout=0.1,
                      pad_vocab_size_multiple=8, fused_dropout_add_ln=True, residual_in_fp32=True).to(_dev()).eval()


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast"])
@pytest.mark.parametrize("B", [1, 4])
def test_lm_lookahead_logits_match_full_forward(gpu_lib, B, autocast):
    L, P, W = 1024, 1024 - 40, 16
    m = _lm(L)
    ids = torch.randint(7, 11, (B, L), generator=torch.Generator().manual_seed(L + B)).to(_dev())
    got, ref = LA.lm_teacher_forced(m, ids, P, W, "cuda" if autocast else None)
    tol = 2e-2 if autocast else 1e-5
    assert got.shape == ref.shape and LA.rel(got, ref) < tol, LA.rel(got, ref)


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast"])
@pytest.mark.parametrize("sampler", ["torch", "device"])
def test_generate_with_lookahead_is_greedy_under_the_full_forward(gpu_lib, sampler, autocast):
    B, P, n_new, W = 2, 900, 11, 4
    m = _lm(P + n_new)
    ids = torch.randint(7, 11, (B, P), generator=torch.Generator().manual_seed(2)).to(_dev())
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast), LA.watched(m) as log:
        out = m.generate(ids, max_length=P + n_new, use_cache=True, lookahead=W, sampler=sampler, return_dict_in_generate=True,
                         output_scores=True, stop_check_every=3 if sampler == "device" else 0)
    log.check_schedule(W, P, n_new)                                        # the lookahead cache did the work: 3 refreshes per layer
    assert out.sequences.shape == (B, P + n_new) and torch.equal(out.sequences[:, :P], ids) and len(out.scores) == n_new
    LA.check_greedy_against_forward(m, out.sequences, P, 2e-2 if autocast else 1e-5, "cuda" if autocast else None)


@pytest.mark.parametrize("sampler,kw", [("torch", {}), ("device", dict(top_k=4, seed=11))], ids=["torch", "device"])
def test_graphed_lookahead_step_is_bitwise_the_eager_one(gpu_lib, sampler, kw):
    """W = 4, 11 new tokens: the replays cross two refreshes; cg against eager, and eager twice, tokens and scores"""
    import hyena_dna_amd
    assert hyena_dna_amd.GRAPH_SAFE
    B, P, n_new, W = 2, 900, 11, 4
    m = _lm(P + n_new)
    ids = torch.randint(7, 11, (B, P), generator=torch.Generator().manual_seed(5)).to(_dev())
    runs = []
    for cg in (False, True, False):
        if sampler == "torch":
            torch.manual_seed(7)
        with torch.autocast("cuda", dtype=torch.bfloat16), LA.watched(m) as log:
            out = m.generate(ids, max_length=P + n_new, use_cache=True, cg=cg, lookahead=W, sampler=sampler, return_dict_in_generate=True,
                             output_scores=True, **kw)
        log.check_schedule(W, P, n_new)            # eager and graphed alike: 3 refreshes per layer, none counted by the warm-up or the capture
        runs.append((out.sequences, torch.stack(out.scores)))
    (s0, l0), (s1, l1), (s2, l2) = runs
    assert s0.shape == (B, P + n_new)
    assert torch.equal(s0, s1) and torch.equal(l0, l1)                # replay == eager lookahead step, bit for bit
    assert torch.equal(s0, s2) and torch.equal(l0, l2)                # and two eager runs from the same seed agree


def test_graphed_step_leaves_the_refresh_bookkeeping(gpu_lib):
    """warm-up and capture leave base, the carry and the host counter as the prefill's refresh left them (W = 1: the second warm-up step
    falls outside the window and is parked), and a replay refreshes first when one is due"""
    from hyena_dna_amd.inference import InferenceParams
    from hyena_dna_amd.lm import GraphedDecodeStep
    B, P, W = 2, 50, 1
    m = _lm(P + 8)
    ids = torch.randint(7, 11, (B, P + 3), generator=torch.Generator().manual_seed(6)).to(_dev())
    with torch.no_grad():
        ip = InferenceParams(max_seqlen=P + 8, max_batch_size=B, lookahead=W)
        ip.key_value_memory_dict = m.allocate_inference_cache(B, P + 8, lookahead=W)
        m(ids[:, :P], inference_params=ip)
        ip.seqlen_offset = P
        states = list(ip.key_value_memory_dict.values())
        keep = [(s.base.clone(), s.carry.clone(), s.pos.clone(), s.tail.clone(), s.la_used) for s in states]
        step = GraphedDecodeStep(m, ip, B)
        try:
            for s, (base, carry, pos, tail, used) in zip(states, keep):
                assert torch.equal(s.base, base) and torch.equal(s.carry, carry) and torch.equal(s.pos, pos) and torch.equal(s.tail, tail)
                assert s.la_used == used == 0 and s.la_external
            got = []
            for i in range(3):
                got.append(step(ids[:, P + i:P + i + 1]).float().clone())
                ip.seqlen_offset += 1
                assert all(s.pos.item() == P + i + 1 and s.base.item() == P + i for s in states)
        finally:
            step.release()
        assert all(not s.la_external for s in states)
        ref = m(ids)[0].logits[:, P:P + 3].float()
    assert LA.rel(torch.stack(got, 1), ref) < 1e-5


def test_failed_graph_capture_leaves_the_caches_eager(gpu_lib):
    """a GraphedDecodeStep that does not come about (here: the sampler's snapshot raises, before the warm-up) leaves no cache in external
    mode, and the mismatch of InferenceParams.lookahead is refused: the next eager step refreshes and counts as if nothing had been tried"""
    from hyena_dna_amd.inference import InferenceParams
    from hyena_dna_amd.lm import GraphedDecodeStep

    class Broken:
        def snapshot(self, steps):
            raise RuntimeError("no snapshot")

    B, P, W = 2, 50, 1
    m = _lm(P + 8)
    ids = torch.randint(7, 11, (B, P + 2), generator=torch.Generator().manual_seed(9)).to(_dev())
    with torch.no_grad():
        ip = InferenceParams(max_seqlen=P + 8, max_batch_size=B, lookahead=W)
        ip.key_value_memory_dict = m.allocate_inference_cache(B, P + 8, lookahead=W)
        m(ids[:, :P], inference_params=ip)
        ip.seqlen_offset = P
        states = list(ip.key_value_memory_dict.values())
        with pytest.raises(RuntimeError, match="no snapshot"):
            GraphedDecodeStep(m, ip, B, sampler=Broken())
        assert all(not s.la_external and s.la_used == 0 and s.pos.item() == P and s.base.item() == P for s in states)
        ip.lookahead = 2
        with pytest.raises(ValueError, match="lookahead"):
            m(ids[:, P:P + 1], inference_params=ip)
        ip.lookahead = W
        got = []
        for i in range(2):                                                    # W = 1: the second step needs its own refresh
            got.append(m(ids[:, P + i:P + i + 1], inference_params=ip)[0].logits[:, -1].float())
            ip.seqlen_offset += 1
            assert all(s.la_used == 1 and s.pos.item() == P + i + 1 and s.base.item() == P + i for s in states)
        ref = m(ids)[0].logits[:, P:P + 2].float()
    assert LA.rel(torch.stack(got, 1), ref) < 1e-5


def test_default_is_todays_path(gpu_lib):
    B, P, n_new = 2, 200, 6
    m = _lm(P + n_new)
    ids = torch.randint(7, 11, (B, P), generator=torch.Generator().manual_seed(3)).to(_dev())
    a = m.generate(ids, max_length=P + n_new, use_cache=True, return_dict_in_generate=True, output_scores=True)
    b = m.generate(ids, max_length=P + n_new, use_cache=True, lookahead=0, return_dict_in_generate=True, output_scores=True)
    assert torch.equal(a.sequences, b.sequences) and all(torch.equal(x, y) for x, y in zip(a.scores, b.scores))
    for kw in ({}, dict(lookahead=0), dict(lookahead=None)):
        for st in m.allocate_inference_cache(B, P + n_new, **kw).values():
            assert st.W == 0 and st.carry is None and st.carry_part is None and st.la_part is None and st.base is None


def test_refusals(gpu_lib):
    B, P = 2, 12
    m = _lm(40)
    ids = torch.randint(7, 11, (B, P), generator=torch.Generator().manual_seed(4)).to(_dev())
    lengths = torch.tensor([P, P - 3], dtype=torch.int32, device=_dev())
    with pytest.raises(ValueError, match="use_cache"):
        m.generate(ids, max_length=P + 4, lookahead=4)
    with pytest.raises(NotImplementedError, match="out of scope"):
        m.generate(ids, max_length=P + 4, use_cache=True, lookahead=4, lengths=lengths)
    with pytest.raises(NotImplementedError, match="out of scope"):
        m.generate(ids, max_length=P + 4, use_cache=True, lookahead=4, num_return_sequences=2)
    st = next(iter(m.allocate_inference_cache(B, 40, lookahead=4).values()))
    with pytest.raises(NotImplementedError, match="out of scope"):
        st.step_block(torch.zeros(B, 3, 3 * 128, device=_dev()))
    assert st.pos.item() == 0 and st.base.item() == 0
