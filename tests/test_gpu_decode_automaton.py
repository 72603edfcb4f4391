"""Automaton-constrained generation on the MI355X (cases and references: tests/decode_automaton_local.py): the two kernels, and the per-token
graph that ends with them -- generate(cg=True, automaton=...) against the eager run, bit for bit."""
import pytest

from tests import decode_automaton_local as DA

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("dtype", DA.DTYPES)
@pytest.mark.parametrize("V,Vlive", DA.SHAPES)
def test_sampler_vs_constrained_kernel_and_restatement(gpu_lib, V, Vlive, dtype):
    DA.case_sampler(gpu_lib, DEV, V, Vlive, dtype)


def test_sampler_more_rows_than_workgroups(gpu_lib):
    import torch
    DA.case_sampler_grid_stride(gpu_lib, DEV, torch.bfloat16)


@pytest.mark.parametrize("dtype", DA.DTYPES)
@pytest.mark.parametrize("V,Vlive", DA.SHAPES)
def test_one_state_automaton_is_the_constrained_kernel_bit_for_bit(gpu_lib, V, Vlive, dtype):
    DA.case_degenerate(gpu_lib, DEV, V, Vlive, dtype)


@pytest.mark.parametrize("dtype", DA.DTYPES)
@pytest.mark.parametrize("V,Vlive", DA.SHAPES)
def test_beam_step_vs_check_beam_and_states(gpu_lib, V, Vlive, dtype):
    DA.case_beam(gpu_lib, DEV, V, Vlive, dtype)


def test_bad_arguments_are_refused(gpu_lib):
    DA.case_abi_refusals(gpu_lib, DEV)


def test_lm_avoided_motif_is_not_written_eager_and_graphed(gpu_lib):
    import hyena_dna_amd
    assert hyena_dna_amd.GRAPH_SAFE
    DA.case_lm_fails_without_the_feature(DEV, graphed=True)


@pytest.mark.parametrize("mode", DA.LM_MODES)
def test_lm_replay_through_the_existing_kernel_eager_and_graphed(gpu_lib, mode):
    DA.case_lm_replay_through_the_existing_kernel(DEV, mode, graphed=True)


def test_lm_rows_are_words_of_the_language(gpu_lib):
    DA.case_lm_membership(DEV, graphed=True)


def test_lm_prompt_boundary(gpu_lib):
    DA.case_lm_prompt_boundary(DEV)


def test_lm_raw_automaton_under_beam_search_eager_and_graphed(gpu_lib):
    DA.case_lm_raw_automaton_beams(DEV, graphed=True)


def test_lm_graph_equals_eager_and_leaves_the_state_right(gpu_lib):
    DA.case_lm_graph_then_eager(DEV)


def test_lm_refusals(gpu_lib):
    DA.case_lm_refusals(DEV)


@pytest.mark.parametrize("mode", DA.LM_MODES + ("beam",))
def test_lm_without_automaton_is_untouched(gpu_lib, mode):
    DA.case_lm_untouched_default(DEV, mode)
