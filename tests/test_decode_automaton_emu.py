"""Automaton-constrained generation under tests/hipemu (cases and references: tests/decode_automaton_local.py), and the host-only cases:
motif_automaton against brute force, the step tables against exhaustive enumeration."""
import os

import pytest

from tests import decode_automaton_local as DA

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SOURCES = [os.path.join(ROOT, "hyena_dna_amd", "csrc", "decode_kernels.h"), os.path.join(ROOT, "include", "hyena_decode.h"),
               os.path.join(ROOT, "hyena_dna_amd", "csrc", "cm.hip")]
DEV = "cpu"


@pytest.fixture()
def auto_emu(emu_backend):
    """the emulation library of emu_backend, rebuilt if the decode kernels are newer than it (build_emu's freshness check does not list them)"""
    from tests.hipemu import build_emu
    if not os.path.exists(build_emu.OUT) or any(os.path.getmtime(f) > os.path.getmtime(build_emu.OUT) for f in NEW_SOURCES):
        build_emu.build(force=True)
        emu_backend._lib = None
    return emu_backend


# ---- host only -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", DA.MOTIF_CASES, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()).replace("'", ""))
def test_motif_automaton_vs_brute_force(kw):
    DA.case_motif_vs_brute_force(kw)


def test_motif_automaton_limits_and_validation():
    DA.case_motif_limits()


@pytest.mark.parametrize("case", range(len(DA.TABLE_CASES)))
def test_step_tables_vs_exhaustive_enumeration(case):
    DA.case_tables_vs_enumeration(*DA.TABLE_CASES[case])


def test_step_tables_position_independent_case():
    DA.case_tables_position_independent()


def test_entry_points_are_declared_and_bound():
    import re
    from hyena_dna_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hyena_decode.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(hyena_\w+)\s*\(", text))
    assert {"hyena_decode_sample_automaton", "hyena_decode_beam_automaton"} <= names
    src = open(_lib.__file__).read()
    assert "L.hyena_decode_sample_automaton.argtypes" in src and "L.hyena_decode_beam_automaton.argtypes" in src
    assert _lib.AUTOMATON_MAX_STATES == 4096 and "#define HYENA_DECODE_AUTOMATON_MAX_STATES 4096" in text


# ---- kernel-local ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DA.DTYPES)
@pytest.mark.parametrize("V,Vlive", DA.SHAPES)
def test_sampler_vs_constrained_kernel_and_restatement(auto_emu, V, Vlive, dtype):
    DA.case_sampler(auto_emu, DEV, V, Vlive, dtype)


def test_sampler_more_rows_than_workgroups(auto_emu):
    import torch
    DA.case_sampler_grid_stride(auto_emu, DEV, torch.bfloat16)


@pytest.mark.parametrize("dtype", DA.DTYPES)
@pytest.mark.parametrize("V,Vlive", DA.SHAPES)
def test_one_state_automaton_is_the_constrained_kernel_bit_for_bit(auto_emu, V, Vlive, dtype):
    DA.case_degenerate(auto_emu, DEV, V, Vlive, dtype)


@pytest.mark.parametrize("dtype", DA.DTYPES)
@pytest.mark.parametrize("V,Vlive", DA.SHAPES)
def test_beam_step_vs_check_beam_and_states(auto_emu, V, Vlive, dtype):
    DA.case_beam(auto_emu, DEV, V, Vlive, dtype)


def test_bad_arguments_are_refused(auto_emu):
    DA.case_abi_refusals(auto_emu, DEV)


# ---- the language model ----------------------------------------------------------------------------------------------------------------------------
def test_lm_avoided_motif_is_not_written(auto_emu):
    DA.case_lm_fails_without_the_feature(DEV, graphed=False)


@pytest.mark.parametrize("mode", DA.LM_MODES)
def test_lm_replay_through_the_existing_kernel(auto_emu, mode):
    DA.case_lm_replay_through_the_existing_kernel(DEV, mode, graphed=False)


def test_lm_rows_are_words_of_the_language(auto_emu):
    DA.case_lm_membership(DEV, graphed=False)


def test_lm_prompt_boundary(auto_emu):
    DA.case_lm_prompt_boundary(DEV)


def test_lm_raw_automaton_under_beam_search(auto_emu):
    DA.case_lm_raw_automaton_beams(DEV, graphed=False)


def test_lm_refusals(auto_emu):
    DA.case_lm_refusals(DEV)


@pytest.mark.parametrize("mode", DA.LM_MODES + ("beam",))
def test_lm_without_automaton_is_untouched(auto_emu, mode):
    DA.case_lm_untouched_default(DEV, mode)
