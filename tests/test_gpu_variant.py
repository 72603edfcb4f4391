"""MI355X: variant effect scoring (csrc/variant_kernels.h, hyena_dna_amd/variants.py, HyenaDNALM.forward_edited_windows / score_variants /
saturation_mutagenesis).  The cases of tests/test_variant_emu.py on the gfx950 library, against the same fp64 references and derived bounds
(tests/variant_local.py), plus the shipped width (D = 256 at T = 1024, run twice and compared bit for bit), the operator on the two-level
long-convolution plan, and the model under bf16 autocast."""
import pytest
import torch

from tests import variant_local as VL

pytestmark = pytest.mark.gpu
dtypes = pytest.mark.parametrize("dtype", VL.DTYPES, ids=VL.NAME.get)


def _dev():
    return torch.device("cuda", 0)


# ---- 5.1 - 5.3: the kernels ----------------------------------------------------------------------------------------------------------------------
@dtypes
@pytest.mark.parametrize("shape", VL.KERNEL_SHAPES + VL.KERNEL_SHAPES_GPU, ids=VL.case_id)
def test_kernels_vs_fp64(gpu_lib, shape, dtype):
    VL.suite_kernels(gpu_lib, _dev(), dtype, *shape, label="gpu")
    if shape in VL.KERNEL_SHAPES_GPU:
        _, a = VL.run_conv(gpu_lib, _dev(), dtype, *shape, seed=7, label="gpu")
        _, b = VL.run_conv(gpu_lib, _dev(), dtype, *shape, seed=7, label="gpu")
        assert VL.same_bits(a, b), "two runs on fresh buffers differ"


@dtypes
def test_rows_are_independent(gpu_lib, dtype):
    VL.run_row_independence(gpu_lib, _dev(), dtype)
    VL.run_row_independence(gpu_lib, _dev(), dtype, D=70, Tn=600, seed=6)       # one channel per workgroup, two pairs per thread


@dtypes
@pytest.mark.parametrize("shape", [(2, 5, 3), (2, 8, 65), (2, 70, 1024)], ids=VL.case_id)
def test_zero_delta_is_the_reference(gpu_lib, shape, dtype):
    VL.run_conv_zero_delta(gpu_lib, _dev(), dtype, *shape)


def test_bad_arguments(gpu_lib):
    VL.check_bad_arguments(gpu_lib, _dev())


# ---- 5.4: the operator -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", VL.OPERATOR_CASES + VL.OPERATOR_CASES_GPU, ids=VL.case_id)
def test_operator_windows_match_forward_over_edited_input(gpu_lib, case):
    VL.run_operator(_dev(), *case, label="gpu")


# ---- 5.5 - 5.7: the model ------------------------------------------------------------------------------------------------------------------------
def test_model_windows_match_full_forwards(gpu_lib):
    VL.run_model_windows(_dev(), 96, (1, 2, 17, 40, 80, 95), 24, VL.TOL, label="gpu")


@pytest.mark.parametrize("d", [64, 128])
def test_model_windows_under_bf16_autocast(gpu_lib, d):
    VL.run_model_windows(_dev(), 4200, (1, 2, 1000, 2047, 4150, 4199), 64, VL.TOL_AUTOCAST, autocast_dev="cuda", d=d, label="gpu autocast")


@pytest.mark.parametrize("L,pos", [(96, 40), (96, 1), (2100, 1000)])
def test_long_convolution_carries_the_effect(gpu_lib, L, pos):
    VL.run_long_conv_carries(_dev(), L, pos, label="gpu")


@pytest.mark.parametrize("L,positions,T", [(96, (1, 2, 40, 70, 71, 95), 24), (96, (5, 60), 64)])
def test_scores_match_full_forward_scores(gpu_lib, L, positions, T):
    VL.run_scores(_dev(), L, positions, T, VL.TOL, label="gpu")


def test_saturation_mutagenesis(gpu_lib):
    VL.run_saturation(_dev(), 96, 30, 36, 16)


# ---- 5.8: refusals -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,message", list(enumerate(VL.REFUSAL_MESSAGES)), ids=[m.replace(" ", "_") for m in VL.REFUSAL_MESSAGES])
def test_refusals(gpu_lib, i, message):
    cases = VL.refusal_cases(_dev())
    assert [c[0] for c in cases] == VL.REFUSAL_MESSAGES
    msg, exc, call = cases[i]
    with pytest.raises(exc, match=message):
        call()
