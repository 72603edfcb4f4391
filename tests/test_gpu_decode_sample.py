"""The device token sampler on the MI355X (cases and reference: tests/decode_sample_local.py), and the per-token graph that ends with it:
generate(sampler="device", cg=True) against the eager device-sampler run, bit for bit."""
import pytest
import torch

from tests import decode_sample_local as DS

pytestmark = pytest.mark.gpu

DEV = "cuda"


def test_uniform_is_the_published_philox_word(gpu_lib):
    DS.case_philox(gpu_lib, DEV)


@pytest.mark.parametrize("dtype", DS.DTYPES)
@pytest.mark.parametrize("V,Vlive", DS.SHAPES)
def test_kernel_vs_fp64_restatement(gpu_lib, V, Vlive, dtype):
    DS.case_kernel_vs_reference(gpu_lib, DEV, V, Vlive, dtype)


@pytest.mark.parametrize("dtype", DS.DTYPES)
@pytest.mark.parametrize("V,Vlive", DS.NF_SHAPES)
def test_nonfinite_logits_rank_first_and_emit_rank_0(gpu_lib, V, Vlive, dtype):
    DS.case_nonfinite(gpu_lib, DEV, V, Vlive, dtype)


@pytest.mark.parametrize("dtype", DS.DTYPES)
def test_clean_rows_after_nonfinite_rows_in_the_grid_stride_loop(gpu_lib, dtype):
    DS.case_nonfinite_grid_stride(gpu_lib, DEV, dtype)


@pytest.mark.parametrize("dtype", DS.DTYPES)
def test_greedy_takes_the_lowest_index_of_equal_maxima(gpu_lib, dtype):
    DS.case_greedy_ties(gpu_lib, DEV, dtype)


def test_draw_frequencies_match_the_probabilities(gpu_lib):
    DS.case_distribution(gpu_lib, DEV)


def test_parked_done_and_eos_rows(gpu_lib):
    DS.case_state(gpu_lib, DEV)


def test_bad_arguments_are_refused(gpu_lib):
    DS.case_refusals(gpu_lib, DEV)


@pytest.mark.parametrize("ragged", [False, True])
def test_lm_device_greedy_is_todays_generate(gpu_lib, ragged):
    DS.case_lm_greedy(DEV, ragged)


@pytest.mark.parametrize("ragged", [False, True])
def test_lm_seeded_sampling_and_live_vocabulary(gpu_lib, ragged):
    DS.case_lm_seeded(DEV, ragged)


@pytest.mark.parametrize("ragged", [False, True])
def test_lm_eos_pads_finished_rows_and_stops_early(gpu_lib, ragged):
    DS.case_lm_eos(DEV, ragged)


def test_lm_refusals(gpu_lib):
    DS.case_lm_refusals(DEV)


@pytest.mark.parametrize("autocast", [False, True])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("kw", [dict(top_k=1, sampler="device"), dict(top_k=4, top_p=0.9, seed=7)], ids=["greedy", "seeded"])
def test_graphed_device_sampler_is_bitwise_the_eager_one(gpu_lib, kw, ragged, autocast):
    import hyena_dna_amd
    assert hyena_dna_amd.GRAPH_SAFE
    m = DS.tiny_lm(DEV)
    ids, lengths = DS.lm_inputs(DEV)
    lengths = lengths if ragged else None
    runs = []
    for cg in (False, True, True):                                             # the second graphed run: a new graph after release()
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            out = DS._gen(m, ids, lengths, cg=cg, **kw)
        assert len(out.scores) == DS.N_LM
        runs.append((out.sequences, torch.stack(out.scores)))
    (s0, l0), (s1, l1), (s2, l2) = runs
    assert torch.equal(s0, s1) and torch.equal(l0, l1)
    assert torch.equal(s0, s2) and torch.equal(l0, l2)
    assert (DS._new_tokens(out, lengths) < 16).all() and (DS._new_tokens(out, lengths) >= 0).all()


def test_graphed_eos_run_is_the_eager_one(gpu_lib):
    """done rows inside the replayed graph: pad goes in as their input, their columns keep pad"""
    m = DS.tiny_lm(DEV)
    ids, lengths = DS.lm_inputs(DEV)
    kw = dict(top_k=4, temperature=1.5, seed=21, vocab_size=12)
    toks = DS._new_tokens(DS._gen(m, ids, lengths, **kw), lengths)
    eos = int(toks[0, 3])
    a = DS._gen(m, ids, lengths, eos_token_id=eos, **kw)
    b = DS._gen(m, ids, lengths, eos_token_id=eos, cg=True, **kw)
    c = DS._gen(m, ids, lengths, eos_token_id=eos, cg=True, stop_check_every=4, **kw)
    assert torch.equal(a.sequences, b.sequences) and torch.equal(torch.stack(a.scores), torch.stack(b.scores))
    assert torch.equal(a.sequences, c.sequences)
    got = DS._new_tokens(b, lengths)
    n = int((toks[0] == eos).nonzero()[0]) + 1
    assert torch.equal(got[0, :n], toks[0, :n]) and (got[0, n:] == DS.PAD).all()
