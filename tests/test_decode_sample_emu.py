"""The device token sampler under tests/hipemu (cases and reference: tests/decode_sample_local.py)."""
import os

import pytest
import torch

from tests import decode_sample_local as DS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SOURCES = [os.path.join(ROOT, "hyena_dna_amd", "csrc", "decode_kernels.h"), os.path.join(ROOT, "include", "hyena_decode.h"),
               os.path.join(ROOT, "hyena_dna_amd", "csrc", "cm.hip")]
DEV = "cpu"


@pytest.fixture()
def sample_emu(emu_backend):
    """the emulation library of emu_backend, rebuilt if the decode kernels are newer than it (build_emu's freshness check does not list them)"""
    from tests.hipemu import build_emu
    if not os.path.exists(build_emu.OUT) or any(os.path.getmtime(f) > os.path.getmtime(build_emu.OUT) for f in NEW_SOURCES):
        build_emu.build(force=True)
        emu_backend._lib = None
    return emu_backend


def test_uniform_is_the_published_philox_word(sample_emu):
    DS.case_philox(sample_emu, DEV)


@pytest.mark.parametrize("dtype", DS.DTYPES)
@pytest.mark.parametrize("V,Vlive", DS.SHAPES)
def test_kernel_vs_fp64_restatement(sample_emu, V, Vlive, dtype):
    DS.case_kernel_vs_reference(sample_emu, DEV, V, Vlive, dtype)


@pytest.mark.parametrize("dtype", DS.DTYPES)
@pytest.mark.parametrize("V,Vlive", DS.NF_SHAPES)
def test_nonfinite_logits_rank_first_and_emit_rank_0(sample_emu, V, Vlive, dtype):
    DS.case_nonfinite(sample_emu, DEV, V, Vlive, dtype)


@pytest.mark.parametrize("dtype", DS.DTYPES)
def test_clean_rows_after_nonfinite_rows_in_the_grid_stride_loop(sample_emu, dtype):
    DS.case_nonfinite_grid_stride(sample_emu, DEV, dtype)


@pytest.mark.parametrize("dtype", DS.DTYPES)
def test_greedy_takes_the_lowest_index_of_equal_maxima(sample_emu, dtype):
    DS.case_greedy_ties(sample_emu, DEV, dtype)


def test_draw_frequencies_match_the_probabilities(sample_emu):
    DS.case_distribution(sample_emu, DEV)


def test_parked_done_and_eos_rows(sample_emu):
    DS.case_state(sample_emu, DEV)


def test_bad_arguments_are_refused(sample_emu):
    DS.case_refusals(sample_emu, DEV)


@pytest.mark.parametrize("ragged", [False, True])
def test_lm_device_greedy_is_todays_generate(sample_emu, ragged):
    DS.case_lm_greedy(DEV, ragged)


@pytest.mark.parametrize("ragged", [False, True])
def test_lm_seeded_sampling_and_live_vocabulary(sample_emu, ragged):
    DS.case_lm_seeded(DEV, ragged)


@pytest.mark.parametrize("ragged", [False, True])
def test_lm_eos_pads_finished_rows_and_stops_early(sample_emu, ragged):
    DS.case_lm_eos(DEV, ragged)


def test_lm_refusals(sample_emu):
    DS.case_lm_refusals(DEV)


def test_device_sampler_refuses_cpu_tensors_on_the_product_backend():
    m = DS.tiny_lm("cpu", n_layer=1)
    ids, _ = DS.lm_inputs("cpu")
    with pytest.raises(NotImplementedError, match="ROCm device"):
        m.generate(ids, max_length=14, use_cache=True, seed=1)


def test_sample_entry_point_is_declared_and_bound():
    import re
    from hyena_dna_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hyena_decode.h")).read(), flags=re.S)
    assert "hyena_decode_sample" in set(re.findall(r"\b(hyena_\w+)\s*\(", text))
    assert "L.hyena_decode_sample.argtypes" in open(_lib.__file__).read()
