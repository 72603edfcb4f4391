"""The lookahead carry (csrc/decode_kernels.h decode_carry / decode_conv_la / decode_post_la, HyenaDecodeState(lookahead=W),
generate(lookahead=W)) on the CPU-emulated kernels: each kernel against the fp64 references and derived bounds of
tests/decode_lookahead_local.py, the cache over two refreshes, HyenaDNALM's teacher-forced logits and greedy generation against the full forward,
the default path and every refusal.  The same cases run on the gfx950 library in tests/test_gpu_decode_lookahead.py."""
import pytest
import torch

from tests import decode_lookahead_local as LA
from tests.test_decode_emu import _lm, decode_emu  # noqa: F401  (the emulation library rebuilt if the decode kernels are newer than it)

DEV = torch.device("cpu")
dtypes = pytest.mark.parametrize("dtype", LA.DTYPES, ids=LA.NAME.get)


# ---- kernels ------------------------------------------------------------------------------------------------------------------------------------
@dtypes
@pytest.mark.parametrize("case", LA.CARRY_CASES, ids=LA.case_id)
def test_carry(decode_emu, case, dtype):  # noqa: F811
    LA.run_carry(decode_emu, DEV, dtype, *case, seed=sum(case), label="emu")


@dtypes
@pytest.mark.parametrize("case", LA.STEP_CASES, ids=LA.case_id)
def test_steps_on_a_carry(decode_emu, case, dtype):  # noqa: F811
    LA.run_steps(decode_emu, DEV, dtype, *case, with_fb=case[0] != 1 or case[1] != 5, seed=sum(case[:5]), label="emu")


@dtypes
def test_step_at_the_end_of_the_cache_is_parked(decode_emu, dtype):  # noqa: F811
    LA.run_parked_with_pre(decode_emu, DEV, dtype, 3, 5, 8260, 8252, 16)


@dtypes
def test_step_past_the_window_parks_all_but_pre(decode_emu, dtype):  # noqa: F811
    LA.run_outside_window_with_pre(decode_emu, DEV, dtype, 3, 5, 8260, 8185, 16)


@dtypes
@pytest.mark.parametrize("case", LA.EQUAL_CASES, ids=LA.case_id)
def test_base_zero_is_the_plain_step(decode_emu, case, dtype):  # noqa: F811
    LA.run_equals_plain(decode_emu, DEV, dtype, *case, seed=sum(case))


def test_bad_arguments(decode_emu):  # noqa: F811
    LA.check_bad_arguments(decode_emu, DEV)


# ---- HyenaDecodeState ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [3, 70, 8190])
def test_state_over_two_refreshes(decode_emu, P):  # noqa: F811
    LA.run_state(DEV, 64, P, W=8, label="emu")


# ---- HyenaDNALM ---------------------------------------------------------------------------------------------------------------------------------
def test_lm_lookahead_logits_match_full_forward(decode_emu):  # noqa: F811
    B, P, N = 2, 45, 12
    m = _lm(P + N)
    ids = torch.randint(7, 11, (B, P + N), generator=torch.Generator().manual_seed(1))
    got, ref = LA.lm_teacher_forced(m, ids, P, 4)
    assert got.shape == ref.shape and LA.rel(got, ref) < 1e-5, LA.rel(got, ref)
    for i in range(ref.shape[1]):
        assert LA.rel(got[:, i], ref[:, i]) < 1e-5, i


@pytest.mark.parametrize("sampler", ["torch", "device"])
def test_generate_with_lookahead_is_greedy_under_the_full_forward(decode_emu, sampler):  # noqa: F811
    B, P, n_new, W = 2, 30, 11, 4
    m = _lm(P + n_new)
    ids = torch.randint(7, 11, (B, P), generator=torch.Generator().manual_seed(2))
    with LA.watched(m) as log:
        out = m.generate(ids, max_length=P + n_new, use_cache=True, lookahead=W, sampler=sampler, return_dict_in_generate=True,
                         output_scores=True, stop_check_every=3 if sampler == "device" else 0)
    log.check_schedule(W, P, n_new)                                        # the lookahead cache did the work: 3 refreshes per layer
    assert out.sequences.shape == (B, P + n_new) and torch.equal(out.sequences[:, :P], ids) and len(out.scores) == n_new
    LA.check_greedy_against_forward(m, out.sequences, P, 1e-5)
    with LA.watched(m) as log:
        again = m.generate(ids, max_length=P + n_new, use_cache=True, lookahead=W, sampler=sampler, return_dict_in_generate=True,
                           output_scores=True)
    log.check_schedule(W, P, n_new)
    assert torch.equal(out.sequences, again.sequences) and all(torch.equal(a, b) for a, b in zip(out.scores, again.scores))


def test_default_is_todays_path(decode_emu):  # noqa: F811
    from hyena_dna_amd.inference import InferenceParams
    B, P, n_new = 2, 20, 6
    m = _lm(P + n_new)
    ids = torch.randint(7, 11, (B, P), generator=torch.Generator().manual_seed(3))
    a = m.generate(ids, max_length=P + n_new, use_cache=True, return_dict_in_generate=True, output_scores=True)
    b = m.generate(ids, max_length=P + n_new, use_cache=True, lookahead=0, return_dict_in_generate=True, output_scores=True)
    c = m.generate(ids, max_length=P + n_new, use_cache=True, lookahead=None, return_dict_in_generate=True, output_scores=True)
    for o in (b, c):
        assert torch.equal(a.sequences, o.sequences) and all(torch.equal(x, y) for x, y in zip(a.scores, o.scores))
    for kw in ({}, dict(lookahead=0), dict(lookahead=None)):
        for st in m.allocate_inference_cache(B, P + n_new, **kw).values():
            assert st.W == 0 and st.carry is None and st.carry_part is None and st.la_part is None and st.base is None
    assert InferenceParams(8, 1).lookahead == 0 and InferenceParams(8, 1, lookahead=4).lookahead == 4
    st = next(iter(m.allocate_inference_cache(B, P + n_new, lookahead=5).values()))
    assert st.W == 5 and st.carry.shape == (B, 5, 64) and st.base.numel() == 1


def test_inference_params_window_is_the_caches(decode_emu):  # noqa: F811
    """InferenceParams.lookahead and the caches' own W cannot disagree: the cached forward refuses the pair before the cache moves"""
    from hyena_dna_amd.inference import InferenceParams
    B, P = 2, 12
    m = _lm(40)
    ids = torch.randint(7, 11, (B, P), generator=torch.Generator().manual_seed(8))
    with torch.no_grad():
        for w_ip, w_cache in ((None, 4), (4, None), (4, 5)):
            ip = InferenceParams(max_seqlen=40, max_batch_size=B, lookahead=w_ip)
            ip.key_value_memory_dict = m.allocate_inference_cache(B, 40, lookahead=w_cache)
            with pytest.raises(ValueError, match="lookahead"):
                m(ids, inference_params=ip)
            assert all(s.pos.item() == 0 for s in ip.key_value_memory_dict.values())
        ip.lookahead = 5                                                     # the same window: served
        m(ids, inference_params=ip)
        ip.lookahead, ip.seqlen_offset = 4, P                                # and a step checks it too
        with pytest.raises(ValueError, match="lookahead"):
            m(ids[:, :1], inference_params=ip)
        assert all(s.pos.item() == P and s.la_used == 0 for s in ip.key_value_memory_dict.values())
        import types                                                         # an object without the attribute (flash_attn's own): the caches' W holds
        m(ids[:, :1], inference_params=types.SimpleNamespace(**{k: v for k, v in vars(ip).items() if k != "lookahead"}))
        assert all(s.pos.item() == P + 1 and s.la_used == 1 for s in ip.key_value_memory_dict.values())


def test_refusals(decode_emu):  # noqa: F811
    from hyena_dna_amd.inference import InferenceParams
    B, P = 2, 12
    m = _lm(40)
    ids = torch.randint(7, 11, (B, P), generator=torch.Generator().manual_seed(4))
    lengths = torch.tensor([P, P - 3], dtype=torch.int32)
    with pytest.raises(ValueError, match="use_cache"):
        m.generate(ids, max_length=P + 4, lookahead=4)
    for kw in (dict(lookahead=65), dict(lookahead=-1)):
        with pytest.raises(ValueError, match="lookahead"):
            m.generate(ids, max_length=P + 4, use_cache=True, **kw)
    for sampler in ("torch", "device"):
        with pytest.raises(NotImplementedError, match="out of scope"):
            m.generate(ids, max_length=P + 4, use_cache=True, lookahead=4, lengths=lengths, sampler=sampler)
        with pytest.raises(NotImplementedError, match="out of scope"):
            m.generate(ids, max_length=P + 4, use_cache=True, lookahead=4, num_return_sequences=2, sampler=sampler)
    with pytest.raises(NotImplementedError, match="out of scope"):
        m.allocate_inference_cache(4, 40, fan=2, prompt_len=P, lookahead=4)
    with pytest.raises(ValueError, match="lookahead"):
        m.allocate_inference_cache(B, 40, lookahead=65)
    # a ragged prefill and an append on a lookahead cache: refused before the cache moves
    with torch.no_grad():
        ip = InferenceParams(max_seqlen=40, max_batch_size=B, lengths_per_sample=lengths, lookahead=4)
        ip.key_value_memory_dict = m.allocate_inference_cache(B, 40, lookahead=4)
        states = list(ip.key_value_memory_dict.values())
        with pytest.raises(NotImplementedError, match="out of scope"):
            m(ids, inference_params=ip)
        assert all(s.pos.item() == 0 and s.base.item() == 0 and not s.ragged for s in states)
        ip.lengths_per_sample = None
        m(ids, inference_params=ip)
        ip.seqlen_offset = P
        ip.allow_append = True
        keep = [(s.pos.clone(), s.base.clone(), s.tail.clone(), s.hist.clone(), s.carry.clone(), s.la_used) for s in states]
        with pytest.raises(NotImplementedError, match="out of scope"):
            m(ids[:, :3], inference_params=ip)
        with pytest.raises(NotImplementedError, match="out of scope"):
            states[0].step_block(torch.zeros(B, 3, 3 * 64))
        for s, (pos, base, tail, hist, carry, used) in zip(states, keep):
            assert torch.equal(s.pos, pos) and torch.equal(s.base, base) and torch.equal(s.tail, tail) and torch.equal(s.hist, hist)
            assert torch.equal(s.carry, carry) and s.la_used == used
        m(ids[:, :1], inference_params=ip)                                   # and the cache still steps
        assert all(s.pos.item() == P + 1 for s in states)
