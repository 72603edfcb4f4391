"""MI355X: NaN, inf and fp16 overflow on the gfx950 library -- the suites of tests/nonfinite_local.py on the device, where the 16-bit store
conversions are the hardware's own (the emulator's are hand-written bit manipulations).  Reads nothing outside the repository.  Counts, run
times, tables and the seeded defects: profiles/nonfinite_local.md."""
import pytest
import torch

from tests import autograd_local as AL
from tests import nonfinite_local as NF

pytestmark = pytest.mark.gpu

_CASES = [(key, i) for key, e in AL.REGISTRY.items() for i in range(len(e.cases(True)))]


def _dev():
    return torch.device("cuda", 0)


@pytest.mark.parametrize("dtype", NF.CVT_DTYPES, ids=[AL.NAME[t] for t in NF.CVT_DTYPES])
def test_store_conversion_over_every_bit_pattern(gpu_lib, dtype):
    NF.suite_cvt_exact(gpu_lib, _dev(), dtype)


@pytest.mark.parametrize("name", list(NF.THRESHOLD))
def test_fp16_overflow_is_stored_as_inf(gpu_lib, name):
    NF.suite_threshold(gpu_lib, _dev(), name)


@pytest.mark.parametrize("key,i", _CASES, ids=[f"{k}-c{i}" for k, i in _CASES])
def test_one_planted_element_propagates_and_stays_in_its_unit(gpu_lib, key, i):
    NF.suite_propagation(gpu_lib, _dev(), key, i, gpu=True)


@pytest.mark.parametrize("dtype", [NF.BF16, NF.F16], ids=["bf16", "fp16"])
def test_mlp_backward_keeps_a_nan_preactivation(gpu_lib, dtype):
    NF.suite_mlp_bwd_nan_preactivation(gpu_lib, _dev(), dtype)


def test_loss_scaler_skips_the_overflowed_step_and_applies_the_clean_one(gpu_lib):
    NF.suite_scaler_steps(gpu_lib, _dev(), gpu=True)


def test_loss_scaler_overflow_is_monotone_in_the_scale(gpu_lib):
    NF.suite_scaler_sweep(gpu_lib, _dev())
