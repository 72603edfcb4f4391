"""NaN, inf and fp16 overflow on the CPU-emulated kernels: the suites of tests/nonfinite_local.py.  tests/test_gpu_nonfinite.py runs the same
suites on the gfx950 library.  Counts, run times, tables and the seeded defects: profiles/nonfinite_local.md."""
import pytest
import torch

from tests import autograd_local as AL
from tests import nonfinite_local as NF

DEV = torch.device("cpu")
_CASES = [(key, i) for key, e in AL.REGISTRY.items() for i in range(len(e.cases(False)))]


@pytest.fixture()
def emu(emu_backend):
    from tests.hipemu import build_emu
    build_emu.build()
    return emu_backend


def test_every_registry_entry_declares_its_unit():
    assert set(NF.UNITS) == set(AL.REGISTRY)
    for key, (kind, act_axes, outs) in NF.UNITS.items():
        assert kind in ("batch", "row", None) and (act_axes is None) == (AL.REGISTRY[key].act is None), key
    for key, n in NF.DISCONNECTED:
        assert n in AL.REGISTRY[key].inputs


@pytest.mark.parametrize("dtype", NF.CVT_DTYPES, ids=[AL.NAME[t] for t in NF.CVT_DTYPES])
def test_store_conversion_over_every_bit_pattern(emu, dtype):
    NF.suite_cvt_exact(emu, DEV, dtype)


@pytest.mark.parametrize("name", list(NF.THRESHOLD))
def test_fp16_overflow_is_stored_as_inf(emu, name):
    NF.suite_threshold(emu, DEV, name)


@pytest.mark.parametrize("key,i", _CASES, ids=[f"{k}-c{i}" for k, i in _CASES])
def test_one_planted_element_propagates_and_stays_in_its_unit(emu, key, i):
    NF.suite_propagation(emu, DEV, key, i)


@pytest.mark.parametrize("dtype", [NF.BF16, NF.F16], ids=["bf16", "fp16"])
def test_mlp_backward_keeps_a_nan_preactivation(emu, dtype):
    NF.suite_mlp_bwd_nan_preactivation(emu, DEV, dtype)


def test_loss_scaler_skips_the_overflowed_step_and_applies_the_clean_one(emu):
    NF.suite_scaler_steps(emu, DEV)


def test_loss_scaler_overflow_is_monotone_in_the_scale(emu):
    NF.suite_scaler_sweep(emu, DEV)
