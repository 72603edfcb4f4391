"""Variant effect scoring (csrc/variant_kernels.h, hyena_dna_amd/variants.py, HyenaDNALM.forward_edited_windows / score_variants /
saturation_mutagenesis) under tests/hipemu: the two kernels against fp64 references with derived bounds, row independence, delta == 0, the
operator's window route against its own forward over the edited input, the model's windows and scores against full forwards of the edited
sequences, and every refusal (tests/variant_local.py)."""
import os

import pytest
import torch

from tests import variant_local as VL

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SOURCES = [os.path.join(ROOT, "hyena_dna_amd", "csrc", "variant_kernels.h"), os.path.join(ROOT, "include", "hyena_variant.h"),
               os.path.join(ROOT, "hyena_dna_amd", "csrc", "cm.hip")]
CPU = torch.device("cpu")
dtypes = pytest.mark.parametrize("dtype", VL.DTYPES, ids=VL.NAME.get)


@pytest.fixture()
def variant_emu(emu_backend):
    """the emulation library of emu_backend, rebuilt if the variant kernels are newer than it (build_emu's freshness check does not list them)"""
    from tests.hipemu import build_emu
    if not os.path.exists(build_emu.OUT) or any(os.path.getmtime(f) > os.path.getmtime(build_emu.OUT) for f in NEW_SOURCES):
        build_emu.build(force=True)
        emu_backend._lib = None
    return emu_backend


# ---- 5.1 - 5.3: the kernels ----------------------------------------------------------------------------------------------------------------------
@dtypes
@pytest.mark.parametrize("shape", VL.KERNEL_SHAPES, ids=VL.case_id)
def test_kernels_vs_fp64(variant_emu, shape, dtype):
    VL.suite_kernels(variant_emu, CPU, dtype, *shape, label="emu")


@dtypes
def test_rows_are_independent(variant_emu, dtype):
    VL.run_row_independence(variant_emu, CPU, dtype)


@dtypes
@pytest.mark.parametrize("shape", [(2, 5, 3), (2, 8, 65)], ids=VL.case_id)
def test_zero_delta_is_the_reference(variant_emu, shape, dtype):
    VL.run_conv_zero_delta(variant_emu, CPU, dtype, *shape)


def test_bad_arguments(variant_emu):
    VL.check_bad_arguments(variant_emu, CPU)


# ---- 5.4: the operator -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", VL.OPERATOR_CASES, ids=VL.case_id)
def test_operator_windows_match_forward_over_edited_input(variant_emu, case):
    VL.run_operator(CPU, *case, label="emu")


# ---- 5.5 - 5.7: the model ------------------------------------------------------------------------------------------------------------------------
def test_model_windows_match_full_forwards(variant_emu):
    VL.run_model_windows(CPU, 96, (1, 2, 17, 40, 80, 95), 24, VL.TOL, label="emu")


@pytest.mark.parametrize("L,pos", [(96, 40), (96, 1), (2100, 1000)])
def test_long_convolution_carries_the_effect(variant_emu, L, pos):
    VL.run_long_conv_carries(CPU, L, pos, label="emu")


@pytest.mark.parametrize("L,positions,T", [(96, (1, 2, 40, 70, 71, 95), 24), (96, (5, 60), 64)])
def test_scores_match_full_forward_scores(variant_emu, L, positions, T):
    VL.run_scores(CPU, L, positions, T, VL.TOL, label="emu")


def test_saturation_mutagenesis(variant_emu):
    VL.run_saturation(CPU, 96, 30, 36, 16)


# ---- 5.8: refusals -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,message", list(enumerate(VL.REFUSAL_MESSAGES)), ids=[m.replace(" ", "_") for m in VL.REFUSAL_MESSAGES])
def test_refusals(variant_emu, i, message):
    cases = VL.refusal_cases(CPU)
    assert [c[0] for c in cases] == VL.REFUSAL_MESSAGES
    msg, exc, call = cases[i]
    with pytest.raises(exc, match=message):
        call()
