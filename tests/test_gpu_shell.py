"""MI355X: the operator's element-wise shell -- the four channel-major kernels of csrc/cm_kernels.h and the eight position-major ones of
csrc/mixer_kernels.h -- each kernel of the gfx950 library called on its own against the element-wise fp64 references and derived bounds of
tests/shell_local.py (evaluated by torch ops on the device): every output element within its bound, every sum of the short filter's
gradients within its own, NaN in every gap of every input, a sentinel in every byte the contract leaves alone, the backward kernels
repeatable bit for bit, the wrappers of _lib on caller-made layouts.  The cases are those of tests/test_shell_emu.py: the smallest shapes
that reach each code path (the workload shapes are the core tests', tests/test_gpu_cm.py).  Figures: profiles/shell_local.md."""
import pytest
import torch

from tests import shell_local as SL

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


@pytest.mark.parametrize("dtype", SL.DTYPES, ids=SL.NAME.get)
@pytest.mark.parametrize("L", SL.CM_LENGTHS)
def test_cm_kernels_at_tile_edges(gpu_lib, L, dtype):
    """lengths round the 8-position vector and the 2048-position tile, each with Lx - L in {0, 1, 2, 3, 11}"""
    for case in SL.cm_length_cases(L):
        SL.run_cm(gpu_lib, _dev(), dtype, label="gpu", **case)


@pytest.mark.parametrize("dtype", SL.DTYPES, ids=SL.NAME.get)
@pytest.mark.parametrize("B,L,rpw", SL.CM_RPW)
def test_cm_kernels_rows_per_workgroup(gpu_lib, B, L, rpw, dtype):
    """1, 2, 4 and 8 rows of one channel per workgroup, ragged last groups included"""
    i = SL.CM_RPW.index((B, L, rpw))
    SL.run_cm(gpu_lib, _dev(), dtype, B, L, L + (i % 2) * 5, 2, xlayout=SL.X_LAYOUTS[i % 3], rows=bool(i % 2), zrows=bool(i % 3 == 1),
              dzrows=bool(i % 3 == 2), bias=True, seed=77 + i, rpw=rpw, label="gpu")


@pytest.mark.parametrize("dtype", SL.DTYPES, ids=SL.NAME.get)
@pytest.mark.parametrize("L", SL.PM_LENGTHS)
@pytest.mark.parametrize("D", SL.PM_NARROW + SL.PM_WIDE)
def test_position_major_kernels(gpu_lib, D, L, dtype):
    """the one-wavefront kernels (any D) and the 256-thread ones (D % 64 == 0) round the 64-position tile and the 1024-position run"""
    for case in SL.pm_cases(D, L):
        SL.run_pm(gpu_lib, _dev(), dtype, label="gpu", **case)


@pytest.mark.parametrize("dtype", SL.DTYPES, ids=SL.NAME.get)
def test_decode_pre_is_cm_pre_fwd_at_one_position(gpu_lib, dtype):
    """bit for bit in fp32; in the 16-bit types at most 2e-5 of the elements on the neighbouring value (16 x 1024 x 4 elements: one)"""
    SL.run_decode_pre(gpu_lib, _dev(), dtype, B=16, D=1024, exact=dtype == torch.float32, label="gpu")
