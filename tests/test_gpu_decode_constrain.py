"""The constrained device sampler on the MI355X (cases and references: tests/decode_constrain_local.py), and the per-token graph that ends
with it: generate(cg=True) with constraints and log-probs against the eager run, bit for bit."""
import pytest

from tests import decode_constrain_local as DC

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("family", DC.FAMILIES)
@pytest.mark.parametrize("dtype", DC.DTYPES)
@pytest.mark.parametrize("V,Vlive", DC.SHAPES)
def test_tokens_vs_fp64_restatement_on_the_allowed_columns(gpu_lib, V, Vlive, dtype, family):
    DC.case_tokens(gpu_lib, DEV, V, Vlive, dtype, family)


@pytest.mark.parametrize("dtype", DC.DTYPES)
@pytest.mark.parametrize("V,Vlive", DC.SHAPES)
def test_no_mask_and_all_ones_are_the_old_kernel_bit_for_bit(gpu_lib, V, Vlive, dtype):
    DC.case_identity_with_old_kernel(gpu_lib, DEV, V, Vlive, dtype)


@pytest.mark.parametrize("dtype", DC.DTYPES)
@pytest.mark.parametrize("V,Vlive", DC.SHAPES)
def test_forced_mask_emits_its_token_whatever_the_logits(gpu_lib, V, Vlive, dtype):
    DC.case_forced(gpu_lib, DEV, V, Vlive, dtype)


def test_parked_and_done_rows_write_nothing_but_pad(gpu_lib):
    DC.case_state(gpu_lib, DEV)


def test_draw_frequencies_under_a_four_token_mask(gpu_lib):
    DC.case_distribution(gpu_lib, DEV)


@pytest.mark.parametrize("dtype", DC.DTYPES)
@pytest.mark.parametrize("V,Vlive", DC.SHAPES)
def test_logprobs_vs_fp64_log_softmax(gpu_lib, V, Vlive, dtype):
    DC.case_logprobs(gpu_lib, DEV, V, Vlive, dtype)


def test_bad_arguments_are_refused(gpu_lib):
    DC.case_abi_refusals(gpu_lib, DEV)


@pytest.mark.parametrize("mode", DC.LM_MODES)
def test_lm_allowed_tokens_and_logprobs_eager_and_graphed(gpu_lib, mode):
    import hyena_dna_amd
    assert hyena_dna_amd.GRAPH_SAFE
    DC.case_lm_allowed_tokens(DEV, mode, graphed=True)


def test_lm_iupac_constraints(gpu_lib):
    DC.case_lm_iupac(DEV, graphed=True)


def test_lm_min_new_tokens_holds_eos_back(gpu_lib):
    DC.case_lm_min_new_tokens(DEV, graphed=True)


@pytest.mark.parametrize("ragged", [False, True])
def test_lm_all_ones_constraints_are_todays_generate(gpu_lib, ragged):
    DC.case_lm_all_ones_is_todays_generate(DEV, ragged)


def test_lm_stop_check_with_logprobs(gpu_lib):
    DC.case_lm_stop_check(DEV)


def test_lm_refusals(gpu_lib):
    DC.case_lm_refusals(DEV)
