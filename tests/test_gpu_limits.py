"""The pitched entry points at their 32-bit offset limits, and three packed calls just past 2^32 bytes, on the device.  Cases, layout and references:
tests/limits_local.py; the table and the figures of one run: profiles/limits_local.md."""
import pytest
import torch

from tests import limits_local as LL

pytestmark = pytest.mark.gpu


@pytest.fixture()
def dev(gpu_lib):
    yield torch.device("cuda", 0)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("i", range(len(LL.FFT_CASES)), ids=LL.FFT_IDS)
def test_fftconv_far_apart_rows(gpu_lib, dev, monkeypatch, i):
    LL.fft_case(gpu_lib, dev, monkeypatch, i, label="gpu")
    assert LL.Rows.held == 0


def test_inproj_vg_pitch_at_its_limit(gpu_lib, dev):
    LL.inproj_case(gpu_lib, dev, torch.bfloat16, label="gpu")
    assert LL.Rows.held == 0


@pytest.mark.parametrize("which", ["lda", "csx"])
def test_cm_rows_across_4_gib(gpu_lib, dev, which):
    LL.cm_case(gpu_lib, dev, torch.bfloat16, which, label="gpu")
    assert LL.Rows.held == 0


@pytest.mark.parametrize("T", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_filter16_rows_at_the_pitch_limit(gpu_lib, dev, T):
    LL.filter16_case(gpu_lib, dev, T, label="gpu")
    assert LL.Rows.held == 0


def test_packed_add_norm_past_2_31_elements(gpu_lib, dev):
    LL.packed_add_norm(gpu_lib, dev, label="gpu")


def test_packed_cm_shell_past_2_32_bytes(gpu_lib, dev):
    LL.packed_cm(gpu_lib, dev, label="gpu")


def test_packed_two_level_fftconv_past_2_32_bytes(gpu_lib, dev, monkeypatch):
    LL.packed_fftconv(gpu_lib, dev, monkeypatch, label="gpu")


def test_filter_rows_at_the_pitch_limit(gpu_lib, dev):
    LL.filter_case(gpu_lib, dev, label="gpu")
    assert LL.Rows.held == 0


@pytest.mark.parametrize("which", ["gen1", "gen2", "dgrad"])
def test_outproj_rows_across_4_gib(gpu_lib, dev, which):
    LL.outproj_case(gpu_lib, dev, torch.float16 if which == "dgrad" else torch.bfloat16, which, label="gpu")
    assert LL.Rows.held == 0


@pytest.mark.parametrize("form", ["single", "rows", "block"])
def test_decode_conv_rows_across_4_gib(gpu_lib, dev, form):
    LL.decode_conv_case(gpu_lib, dev, torch.bfloat16, form, label="gpu")
    assert LL.Rows.held == 0
