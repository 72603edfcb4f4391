"""The fp32 implicit-filter kernels of the gfx950 library (csrc/filter_kernels.h) element by element against the layer-local fp64 references of
tests/filter_local.py, evaluated on the device: the cases of tests/test_filter_local_emu.py plus the one the emulator cannot afford -- 258
workgroup iterations on 256 workgroups.  Every buffer is sized as include/hyena_filter.h says.  Figures: profiles/filter_local.md."""
import pytest
import torch

from tests import filter_local as FLoc
from tests.test_filter_local_emu import CASES, HUGE_CASE, LONG_CASES, run_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES + LONG_CASES + [HUGE_CASE], ids=lambda c: f"D{c[0]}-L{c[1]}-E{c[2]}-ldk{c[3]}-zs{c[4]}")
def test_filter_layer_local_vs_fp64(gpu_lib, case):
    run_case(gpu_lib, case, device="cuda", label="gfx950")


@pytest.mark.parametrize("kw", [{"modulate": False}, {"need_dz": False}], ids=["nomod", "nodz"])
def test_filter_layer_local_strided_z_options(gpu_lib, kw):
    """z_stride = 8 > E = 5 with NaN in the unused columns, without the modulation and without dz"""
    run_case(gpu_lib, CASES[-1], device="cuda", label="gfx950", **kw)


def test_modulation_probe(gpu_lib):
    """eps_m of v_exp_f32 behind an fp32 product, through the ABI: what a 1 - 2 ulp exp2 explains (2 ulp at the bottom of a binade = 4 u)"""
    eps, info = FLoc.modulation_probe(gpu_lib, torch.device("cuda"))
    print(f"[filter-local] gfx950 eps_m measured {eps:.3g} = {eps / FLoc.U:.2f} u; {info}")
    assert info["samples"] > 0.5 * 256 * 2048 and info["max_t_delta"] > 80
    assert eps <= FLoc.EPS_M_CAP, eps
