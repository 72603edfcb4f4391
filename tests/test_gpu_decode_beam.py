"""Beam search for cached generation on the MI355X (cases and references: tests/decode_beam_local.py), plus the wide reorder, the long
prompt (S > 0) and the per-token graph that ends with the beam step and the caches' re-parenting."""
import pytest
import torch

from tests import decode_beam_local as DB

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("dtype", DB.DTYPES)
@pytest.mark.parametrize("shape", DB.REORDER_SHAPES + [DB.REORDER_SHAPE_WIDE])
def test_reorder_equals_index_select_and_touches_nothing_else(gpu_lib, shape, dtype):
    DB.case_reorder(gpu_lib, DEV, shape, dtype)


@pytest.mark.parametrize("dtype", DB.DTYPES)
def test_reorder_at_a_position_outside_the_cache_changes_nothing(gpu_lib, dtype):
    DB.case_reorder_parked(gpu_lib, DEV, dtype)


def test_reorder_refuses_bad_arguments(gpu_lib):
    DB.case_reorder_refusals(gpu_lib, DEV)


@pytest.mark.parametrize("dtype", DB.DTYPES)
@pytest.mark.parametrize("V,Vlive", DB.VSHAPES)
def test_beam_step_vs_fp64_restatement(gpu_lib, V, Vlive, dtype):
    DB.case_beam(gpu_lib, DEV, V, Vlive, dtype)


@pytest.mark.parametrize("dtype", DB.DTYPES)
def test_beam_step_ranks_bit_equal_scores_by_flat_index(gpu_lib, dtype):
    DB.case_beam_ties(gpu_lib, DEV, dtype)


@pytest.mark.parametrize("dtype", DB.DTYPES)
@pytest.mark.parametrize("V,Vlive", DB.VSHAPES)
def test_beam_step_is_total_on_nonfinite_logits(gpu_lib, V, Vlive, dtype):
    DB.case_beam_nonfinite(gpu_lib, DEV, V, Vlive, dtype)


def test_beam_and_backtrack_refuse_bad_arguments(gpu_lib):
    DB.case_beam_refusals(gpu_lib, DEV)


def test_backtrack_walks_the_records(gpu_lib):
    DB.case_backtrack(gpu_lib, DEV)


@pytest.mark.parametrize("P", [3, 8190 + 7])
def test_reorder_inside_a_live_cache_equals_replaying_each_lineage(gpu_lib, P):
    DB.case_operator_reorder(DEV, P)


def test_reorder_refusals(gpu_lib):
    DB.case_state_refusals(DEV)


def test_lm_exhaustive_search_finds_every_continuation_and_the_best(gpu_lib):
    DB.case_lm_exhaustive(DEV)


@pytest.mark.parametrize("P,d", [(40, 64), (8192 + 5, 128)])
def test_lm_pruning_search_scores_are_teacher_forced_scores(gpu_lib, P, d):
    DB.case_lm_pruning(DEV, P=P, d=d)


def test_lm_pruning_search_under_autocast(gpu_lib):
    DB.case_lm_pruning(DEV, P=40, d=128, autocast=torch.bfloat16)


def test_lm_constraints(gpu_lib):
    DB.case_lm_constraints(DEV)


def test_lm_eos_and_stop_check(gpu_lib):
    DB.case_lm_eos(DEV)


def test_lm_one_beam_is_todays_generate(gpu_lib):
    DB.case_lm_one_beam_is_todays_generate(DEV)


def test_lm_refusals(gpu_lib):
    DB.case_lm_refusals(DEV)


@pytest.mark.parametrize("P,d", [(40, 64), (8192 + 5, 128)])
def test_lm_graphed_search_equals_eager_bit_for_bit(gpu_lib, P, d):
    import hyena_dna_amd
    assert hyena_dna_amd.GRAPH_SAFE
    DB.case_lm_graph_equals_eager(DEV, P=P, d=d)
