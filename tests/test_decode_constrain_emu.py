"""The constrained device sampler under tests/hipemu (cases and references: tests/decode_constrain_local.py), and the host-only mask helpers."""
import os

import pytest
import torch

from tests import decode_constrain_local as DC

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


@pytest.mark.parametrize("family", DC.FAMILIES)
@pytest.mark.parametrize("dtype", DC.DTYPES)
@pytest.mark.parametrize("V,Vlive", DC.SHAPES)
def test_tokens_vs_fp64_restatement_on_the_allowed_columns(sample_emu, V, Vlive, dtype, family):
    DC.case_tokens(sample_emu, DEV, V, Vlive, dtype, family)


@pytest.mark.parametrize("dtype", DC.DTYPES)
@pytest.mark.parametrize("V,Vlive", DC.SHAPES)
def test_no_mask_and_all_ones_are_the_old_kernel_bit_for_bit(sample_emu, V, Vlive, dtype):
    DC.case_identity_with_old_kernel(sample_emu, DEV, V, Vlive, dtype)


@pytest.mark.parametrize("dtype", DC.DTYPES)
@pytest.mark.parametrize("V,Vlive", DC.SHAPES)
def test_forced_mask_emits_its_token_whatever_the_logits(sample_emu, V, Vlive, dtype):
    DC.case_forced(sample_emu, DEV, V, Vlive, dtype)


def test_parked_and_done_rows_write_nothing_but_pad(sample_emu):
    DC.case_state(sample_emu, DEV)


def test_draw_frequencies_under_a_four_token_mask(sample_emu):
    DC.case_distribution(sample_emu, DEV)


@pytest.mark.parametrize("dtype", DC.DTYPES)
@pytest.mark.parametrize("V,Vlive", DC.SHAPES)
def test_logprobs_vs_fp64_log_softmax(sample_emu, V, Vlive, dtype):
    DC.case_logprobs(sample_emu, DEV, V, Vlive, dtype)


def test_bad_arguments_are_refused(sample_emu):
    DC.case_abi_refusals(sample_emu, DEV)


@pytest.mark.parametrize("mode", DC.LM_MODES)
def test_lm_allowed_tokens_and_logprobs(sample_emu, mode):
    DC.case_lm_allowed_tokens(DEV, mode, graphed=False)


def test_lm_iupac_constraints(sample_emu):
    DC.case_lm_iupac(DEV, graphed=False)


def test_lm_min_new_tokens_holds_eos_back(sample_emu):
    DC.case_lm_min_new_tokens(DEV, graphed=False)


@pytest.mark.parametrize("ragged", [False, True])
def test_lm_all_ones_constraints_are_todays_generate(sample_emu, ragged):
    DC.case_lm_all_ones_is_todays_generate(DEV, ragged)


def test_lm_stop_check_with_logprobs(sample_emu):
    DC.case_lm_stop_check(DEV)


def test_lm_refusals(sample_emu):
    DC.case_lm_refusals(DEV)


# ---- host only -------------------------------------------------------------------------------------------------------------------------------------
def test_token_mask():
    from hyena_dna_amd.inference import token_mask
    assert token_mask([]) == 0 and token_mask([0]) == 1 and token_mask([7, 8, 9, 10]) == 0xF << 7 and token_mask((3, 3, 5)) == 0b101000
    assert token_mask([63]) == -2 ** 63 and token_mask(range(64)) == -1 and token_mask(range(63)) == 2 ** 63 - 1
    assert torch.tensor([token_mask([63, 0])], dtype=torch.int64).item() == -2 ** 63 + 1      # fits an int64 tensor as it is
    assert isinstance(token_mask(torch.tensor([1, 2])), int) and token_mask(torch.tensor([1, 2])) == 6
    for bad in ([64], [-1], [3, 100]):
        with pytest.raises(ValueError, match="token id"):
            token_mask(bad)


def test_iupac_constraints():
    from hyena_dna_amd.inference import iupac_constraints, token_mask
    from hyena_dna_amd.tokenizer import DNACharTokenizerLUT
    tok = DNACharTokenizerLUT().vocab
    assert [tok[c] for c in "ACGT"] == [7, 8, 9, 10]
    c = iupac_constraints("ACGT.NRYSWKMBDHV")
    assert c.dtype == torch.int64 and c.shape == (16,) and c.device.type == "cpu"
    sets = dict(A="A", C="C", G="G", T="T", N="ACGT", R="AG", Y="CT", S="CG", W="AT", K="GT", M="AC", B="CGT", D="AGT", H="ACT", V="ACG")
    for ch, m in zip("ACGT.NRYSWKMBDHV", c.tolist()):
        assert m == (-1 if ch == "." else token_mask(tok[b] for b in sets[ch])), ch
    assert torch.equal(iupac_constraints("acgtn"), iupac_constraints("ACGTN"))
    assert iupac_constraints("").shape == (0,)
    other = iupac_constraints("AY", token_of=dict(A=0, C=1, G=2, T=63))
    assert other.tolist() == [1, 2 - 2 ** 63]
    with pytest.raises(ValueError, match=r"pattern\[2\]"):
        iupac_constraints("ACXT")


def test_constrained_entry_point_is_declared_and_bound():
    import re
    from hyena_dna_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hyena_decode.h")).read(), flags=re.S)
    assert "hyena_decode_sample_constrained" in set(re.findall(r"\b(hyena_\w+)\s*\(", text))
    assert "L.hyena_decode_sample_constrained.argtypes" in open(_lib.__file__).read()
