"""MI355X: the decode kernels of csrc/decode_kernels.h -- conv and post of the four families, pre of the three variants -- each kernel of the
gfx950 library called on its own against the element-wise fp64 references and derived bounds of tests/decode_local.py (evaluated by torch ops on
the device).  The suites are those of tests/test_decode_local_emu.py, plus one call per conv and post form at the shipped width (D = 256, B = 4,
a grid of 3 x 256 workgroups), run twice on fresh buffers and compared bit for bit.  Figures: profiles/decode_local.md."""
import pytest
import torch

from tests import decode_local as DL

pytestmark = pytest.mark.gpu
dtypes = pytest.mark.parametrize("dtype", DL.DTYPES, ids=DL.NAME.get)


def _dev():
    return torch.device("cuda", 0)


@dtypes
@pytest.mark.parametrize("Lcap,ts", DL.CONV_SINGLE, ids=lambda v: str(v) if isinstance(v, int) else f"t{v[0]}")
def test_conv_single(gpu_lib, Lcap, ts, dtype):
    DL.suite_conv_single(gpu_lib, _dev(), dtype, Lcap, ts, "gpu")


@dtypes
@pytest.mark.parametrize("t", DL.CONV_SINGLE_LONG)
def test_conv_single_at_2_20(gpu_lib, t, dtype):
    DL.suite_conv_single_long(gpu_lib, _dev(), dtype, t, "gpu")


@dtypes
def test_conv_rows(gpu_lib, dtype):
    DL.suite_conv_rows(gpu_lib, _dev(), dtype, "gpu")


@dtypes
@pytest.mark.parametrize("S", DL.FAN_S)
def test_conv_fan(gpu_lib, S, dtype):
    DL.suite_conv_fan(gpu_lib, _dev(), dtype, S, "gpu")


@dtypes
@pytest.mark.parametrize("T", DL.BLOCK_T)
def test_conv_block(gpu_lib, T, dtype):
    DL.suite_conv_block(gpu_lib, _dev(), dtype, T, "gpu")


@dtypes
@pytest.mark.parametrize("with_fb", [True, False], ids=["fb", "nofb"])
@pytest.mark.parametrize("form", DL.FORMS)
def test_post(gpu_lib, form, with_fb, dtype):
    DL.suite_post(gpu_lib, _dev(), dtype, form, with_fb, "gpu")


@dtypes
@pytest.mark.parametrize("bias", [True, False], ids=["bin", "nobin"])
@pytest.mark.parametrize("form", ["rows", "fan", "block"])
def test_pre_variants(gpu_lib, form, bias, dtype):
    DL.suite_pre(gpu_lib, _dev(), dtype, form, bias, "gpu")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=DL.NAME.get)
@pytest.mark.parametrize("form", DL.FORMS)
@pytest.mark.parametrize("kind", ["conv", "post"])
def test_shipped_width_twice(gpu_lib, kind, form, dtype):
    DL.suite_wide(gpu_lib, _dev(), dtype, kind, form, "gpu-wide")
