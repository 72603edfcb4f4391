"""The operator's element-wise shell -- the four channel-major kernels of csrc/cm_kernels.h and the eight position-major ones of
csrc/mixer_kernels.h -- on the CPU-emulated kernels, each kernel called on its own against the element-wise fp64 references and derived
bounds of tests/shell_local.py: every output element within its bound, every sum of the short filter's gradients within its own, NaN in
every gap of every input, a sentinel in every byte the contract leaves alone, the backward kernels repeatable bit for bit, the wrappers of
_lib on caller-made layouts.  The same checks run on the gfx950 library in tests/test_gpu_shell.py; figures of both in
profiles/shell_local.md."""
import pytest
import torch

from tests import shell_local as SL
from tests.test_decode_emu import decode_emu  # noqa: F401  (the emulation library rebuilt if the decode kernels are newer than it)

DEV = torch.device("cpu")


@pytest.mark.parametrize("dtype", SL.DTYPES, ids=SL.NAME.get)
@pytest.mark.parametrize("L", SL.CM_LENGTHS)
def test_cm_kernels_at_tile_edges(emu_backend, L, dtype):
    """lengths round the 8-position vector and the 2048-position tile, each with Lx - L in {0, 1, 2, 3, 11}"""
    for case in SL.cm_length_cases(L):
        SL.run_cm(emu_backend, DEV, dtype, label="emu", **case)


@pytest.mark.parametrize("dtype", SL.DTYPES, ids=SL.NAME.get)
@pytest.mark.parametrize("B,L,rpw", SL.CM_RPW)
def test_cm_kernels_rows_per_workgroup(emu_backend, B, L, rpw, dtype):
    """1, 2, 4 and 8 rows of one channel per workgroup, ragged last groups included"""
    i = SL.CM_RPW.index((B, L, rpw))
    SL.run_cm(emu_backend, DEV, dtype, B, L, L + (i % 2) * 5, 2, xlayout=SL.X_LAYOUTS[i % 3], rows=bool(i % 2), zrows=bool(i % 3 == 1),
              dzrows=bool(i % 3 == 2), bias=True, seed=77 + i, rpw=rpw, label="emu")


@pytest.mark.parametrize("dtype", SL.DTYPES, ids=SL.NAME.get)
@pytest.mark.parametrize("L", SL.PM_LENGTHS)
@pytest.mark.parametrize("D", SL.PM_NARROW + SL.PM_WIDE)
def test_position_major_kernels(emu_backend, D, L, dtype):
    """the one-wavefront kernels (any D) and the 256-thread ones (D % 64 == 0) round the 64-position tile and the 1024-position run"""
    for case in SL.pm_cases(D, L):
        SL.run_pm(emu_backend, DEV, dtype, label="emu", **case)


@pytest.mark.parametrize("dtype", SL.DTYPES, ids=SL.NAME.get)
def test_decode_pre_is_cm_pre_fwd_at_one_position(decode_emu, dtype):  # noqa: F811
    SL.run_decode_pre(decode_emu, DEV, dtype, B=3, D=70, exact=True, label="emu")


def test_references_agree_with_autograd():
    """the fp64 references themselves, independent of any kernel: the gradients are autograd's of the forward references"""
    g = torch.Generator().manual_seed(5)
    D, B, L, Lx = 2, 3, 11, 13
    x = torch.randn(3 * D, B, Lx, generator=g, dtype=torch.float64, requires_grad=True)
    bin_ = torch.randn(3 * D, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(3 * D, 3, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(3 * D, generator=g, dtype=torch.float64, requires_grad=True)
    y, dvg = torch.randn(B, D, L, generator=g, dtype=torch.float64), torch.randn(B, D, L, generator=g, dtype=torch.float64)
    dz = torch.randn(D, B, L, generator=g, dtype=torch.float64)
    vg, _ = SL.pre_fwd64(x, bin_, w, b, L)
    z, _ = SL.post_fwd64(x, bin_, w, b, y, L)
    gx, gbin, gw, gb = torch.autograd.grad((vg * dvg).sum() + (z * dz).sum(), (x, bin_, w, b))
    with torch.no_grad():
        R0, R1 = SL.post_bwd64(x, bin_, w, b, y, dz, L), SL.pre_bwd64(x, bin_, w, b, dvg, L)
        sums = torch.cat([R0["sums"], R1["sums"]], 0)
        assert torch.allclose(torch.cat([R0["dx"], R1["dx"]], 0), gx[..., :L], rtol=1e-12, atol=1e-12) and not bool(gx[..., L:].any())
        assert torch.allclose(sums[:, :3], gw, rtol=1e-12, atol=1e-12) and torch.allclose(sums[:, 3], gb, rtol=1e-12, atol=1e-12)
        assert torch.allclose(sums[:, 4], gbin, rtol=1e-12, atol=1e-12)
        # taps before position 0 contribute zero, not bin
        assert torch.allclose(SL.sc64(x, bin_, w, b)[..., 0], b[:, None] + w[:, 2, None] * (x[..., 0] + bin_[:, None]))
        assert (R0["S"] >= sums[:D].abs() - 1e-12).all() and (R1["S"] >= sums[D:].abs() - 1e-12).all()
