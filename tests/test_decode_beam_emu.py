"""Beam search for cached generation under tests/hipemu (cases and references: tests/decode_beam_local.py): the beam step, the fan-out
cache's re-parenting, the backtrack, HyenaDecodeState.reorder inside a live cache, and generate(num_beams=k)."""
import os

import pytest
import torch

from tests import decode_beam_local as DB

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SOURCES = [os.path.join(ROOT, "hyena_dna_amd", "csrc", "decode_kernels.h"), os.path.join(ROOT, "include", "hyena_decode.h"),
               os.path.join(ROOT, "hyena_dna_amd", "csrc", "cm.hip")]
DEV = "cpu"


@pytest.fixture()
def beam_emu(emu_backend):
    """the emulation library of emu_backend, rebuilt if the decode kernels are newer than it (build_emu's freshness check does not list them)"""
    from tests.hipemu import build_emu
    if not os.path.exists(build_emu.OUT) or any(os.path.getmtime(f) > os.path.getmtime(build_emu.OUT) for f in NEW_SOURCES):
        build_emu.build(force=True)
        emu_backend._lib = None
    return emu_backend


# ---- the reorder kernel ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DB.DTYPES)
@pytest.mark.parametrize("shape", DB.REORDER_SHAPES)
def test_reorder_equals_index_select_and_touches_nothing_else(beam_emu, shape, dtype):
    DB.case_reorder(beam_emu, DEV, shape, dtype)


@pytest.mark.parametrize("dtype", DB.DTYPES)
def test_reorder_at_a_position_outside_the_cache_changes_nothing(beam_emu, dtype):
    DB.case_reorder_parked(beam_emu, DEV, dtype)


def test_reorder_refuses_bad_arguments(beam_emu):
    DB.case_reorder_refusals(beam_emu, DEV)


# ---- the beam kernel ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DB.DTYPES)
@pytest.mark.parametrize("V,Vlive", DB.VSHAPES)
def test_beam_step_vs_fp64_restatement(beam_emu, V, Vlive, dtype):
    DB.case_beam(beam_emu, DEV, V, Vlive, dtype)


@pytest.mark.parametrize("dtype", DB.DTYPES)
def test_beam_step_ranks_bit_equal_scores_by_flat_index(beam_emu, dtype):
    DB.case_beam_ties(beam_emu, DEV, dtype)


@pytest.mark.parametrize("dtype", DB.DTYPES)
@pytest.mark.parametrize("V,Vlive", DB.VSHAPES)
def test_beam_step_is_total_on_nonfinite_logits(beam_emu, V, Vlive, dtype):
    DB.case_beam_nonfinite(beam_emu, DEV, V, Vlive, dtype)


def test_beam_and_backtrack_refuse_bad_arguments(beam_emu):
    DB.case_beam_refusals(beam_emu, DEV)


def test_backtrack_walks_the_records(beam_emu):
    DB.case_backtrack(beam_emu, DEV)


# ---- the operator's cache -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [3, 8190 + 7])
def test_reorder_inside_a_live_cache_equals_replaying_each_lineage(beam_emu, P):
    DB.case_operator_reorder(DEV, P)


def test_reorder_refusals(beam_emu):
    DB.case_state_refusals(DEV)


# ---- the language model ---------------------------------------------------------------------------------------------------------------------------
def test_lm_exhaustive_search_finds_every_continuation_and_the_best(beam_emu):
    DB.case_lm_exhaustive(DEV)


def test_lm_pruning_search_scores_are_teacher_forced_scores(beam_emu):
    DB.case_lm_pruning(DEV)


def test_lm_constraints(beam_emu):
    DB.case_lm_constraints(DEV)


def test_lm_eos_and_stop_check(beam_emu):
    DB.case_lm_eos(DEV)


def test_lm_one_beam_is_todays_generate(beam_emu):
    DB.case_lm_one_beam_is_todays_generate(DEV)


def test_lm_refusals(beam_emu):
    DB.case_lm_refusals(DEV)


# ---- host only ------------------------------------------------------------------------------------------------------------------------------------
def test_beam_entry_points_are_declared_and_bound():
    import re
    from hyena_dna_amd import _lib
    text = open(os.path.join(ROOT, "include", "hyena_decode.h")).read()
    assert int(re.search(r"#define HYENA_DECODE_BEAM_MAX (\d+)", text).group(1)) == _lib.DECODE_BEAM_MAX == 16
    declared = set(re.findall(r"\b(hyena_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    src = open(_lib.__file__).read()
    for name in ("hyena_decode_beam", "hyena_decode_reorder_fan", "hyena_decode_beam_backtrack"):
        assert name in declared and f"L.{name}.argtypes" in src
