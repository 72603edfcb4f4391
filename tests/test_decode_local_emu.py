"""The decode kernels of csrc/decode_kernels.h on the CPU-emulated kernels, each called on its own against the element-wise fp64 references and
derived bounds of tests/decode_local.py: every written slot of `part` within gamma_40 sum|k vg| of its own chunk's sum and every other slot bitwise
untouched, z within the bound of two roundings and a gate on caller-made partials, the pre kernels of the variants against sc64 with an exact tail;
NaN wherever nothing may be read, a sentinel wherever nothing may be written, a margin below 1 wherever the operands are flat.  The same suites run
on the gfx950 library in tests/test_gpu_decode_local.py; figures of both and the seeded defects in profiles/decode_local.md."""
import pytest
import torch

from tests import decode_local as DL
from tests.test_decode_emu import decode_emu  # noqa: F401  (the emulation library rebuilt if the decode kernels are newer than it)

DEV = torch.device("cpu")
dtypes = pytest.mark.parametrize("dtype", DL.DTYPES, ids=DL.NAME.get)


@dtypes
@pytest.mark.parametrize("Lcap,ts", DL.CONV_SINGLE, ids=lambda v: str(v) if isinstance(v, int) else f"t{v[0]}")
def test_conv_single(decode_emu, Lcap, ts, dtype):  # noqa: F811
    DL.suite_conv_single(decode_emu, DEV, dtype, Lcap, ts, "emu")


@dtypes
@pytest.mark.parametrize("t", DL.CONV_SINGLE_LONG)
def test_conv_single_at_2_20(decode_emu, t, dtype):  # noqa: F811
    DL.suite_conv_single_long(decode_emu, DEV, dtype, t, "emu")


@dtypes
def test_conv_rows(decode_emu, dtype):  # noqa: F811
    DL.suite_conv_rows(decode_emu, DEV, dtype, "emu")


@dtypes
@pytest.mark.parametrize("S", DL.FAN_S)
def test_conv_fan(decode_emu, S, dtype):  # noqa: F811
    DL.suite_conv_fan(decode_emu, DEV, dtype, S, "emu")


@dtypes
@pytest.mark.parametrize("T", DL.BLOCK_T)
def test_conv_block(decode_emu, T, dtype):  # noqa: F811
    DL.suite_conv_block(decode_emu, DEV, dtype, T, "emu")


@dtypes
@pytest.mark.parametrize("with_fb", [True, False], ids=["fb", "nofb"])
@pytest.mark.parametrize("form", DL.FORMS)
def test_post(decode_emu, form, with_fb, dtype):  # noqa: F811
    DL.suite_post(decode_emu, DEV, dtype, form, with_fb, "emu")


@dtypes
@pytest.mark.parametrize("bias", [True, False], ids=["bin", "nobin"])
@pytest.mark.parametrize("form", ["rows", "fan", "block"])
def test_pre_variants(decode_emu, form, bias, dtype):  # noqa: F811
    DL.suite_pre(decode_emu, DEV, dtype, form, bias, "emu")


def test_references_against_plain_loops():
    """the fp64 references themselves, independent of any kernel: conv_ref against a double loop, post_bound against its parts"""
    g = torch.Generator().manual_seed(3)
    D, R, n, t0, T, s0 = 2, 2, 13, 20, 5, 16
    k = torch.randn(D, 40, generator=g, dtype=torch.float64)
    h = torch.randn(R, D, n, generator=g, dtype=torch.float64)
    ref, S = DL.conv_ref(k, h, t0, T, s0)
    for r in range(R):
        for i in range(T):
            for d in range(D):
                terms = [k[d, t0 + i - s] * h[r, d, s - s0] for s in range(s0, s0 + n) if s <= t0 + i]
                assert abs(float(sum(terms)) - float(ref[r, i, d])) < 1e-12 and abs(float(sum(abs(x) for x in terms)) - float(S[r, i, d])) < 1e-12
    one = torch.ones(1, dtype=torch.float64)
    assert float(DL.post_bound(3 * one, 3 * one, one, one, torch.float32)) == pytest.approx(DL.gamma(2) * 3 + DL.U * 3, rel=1e-6)
    b16 = float(DL.post_bound(3 * one, 3 * one, one, one, torch.bfloat16))                # half an ulp of bf16 at 3 is 2^-7, twice
    assert 2 * 2.0 ** -7 < b16 < 2 * 2.0 ** -7 * 1.01
