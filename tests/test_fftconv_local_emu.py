"""The long convolution on the CPU-emulated kernels against the element-wise fp64 references and bounds of tests/fftconv_local.py, every case
asserting the kernels it reaches: the two-level column kernels of all 30 column sizes (table A: the largest, M1 = 1024, takes 1.5 s per
emulated case, so no M1 is left to the GPU alone), the two-level row kernels and host loop (B), the workspace-free plan under every knob (C)
and its probes, the pitched rows with guards (D).  Only the side-stream switch (E: the emulation has no streams) runs on the GPU alone, in
tests/test_gpu_fftconv_local.py, which runs all of this on the gfx950 library.  Figures: profiles/fftconv_local.md."""
import pytest
import torch

from oracle import hyena_oracle as O
from tests import fftconv_local as FL

DEV = torch.device("cpu")
ids = FL.NAME.get


_A = [(M1, kind, T) for M1, kind in FL.A_PARAMS for T in FL.DTYPES if kind == "ragged" or T != FL.F16]


@pytest.mark.parametrize("M1,kind,dtype", _A, ids=lambda v: FL.NAME[v] if isinstance(v, torch.dtype) else str(v))
def test_column_kernels(emu_backend, monkeypatch, M1, kind, dtype):
    FL.suite_columns(emu_backend, DEV, monkeypatch, dtype, M1, kind, "emu")


@pytest.mark.parametrize("i", range(len(FL.B_CASES)), ids=lambda i: "M1_{}-B{}-chunk{}-need{}{}-saved{}-bias{}-{}".format(
    *FL.B_CASES[i][:3], *FL.B_CASES[i][3], *FL.B_CASES[i][4:6], FL.NAME[FL.B_CASES[i][6]]))
def test_row_kernels_and_host_loop(emu_backend, monkeypatch, i):
    FL.suite_rows(emu_backend, DEV, monkeypatch, i, "emu")


_C = [(i, T) for i, c in enumerate(FL.C_CASES) for T in c[7]]


@pytest.mark.parametrize("i,dtype", _C, ids=lambda v: FL.NAME[v] if isinstance(v, torch.dtype) else "c{}-R{}-B{}-D{}-L{}".format(v, *FL.C_CASES[v][:4]))
def test_workspace_free_plan(emu_backend, monkeypatch, i, dtype):
    FL.suite_onchip(emu_backend, DEV, monkeypatch, i, dtype, "emu")


@pytest.mark.parametrize("dtype", [FL.F32, FL.BF16], ids=ids)
@pytest.mark.parametrize("i", range(len(FL.C_PROBES)))
def test_workspace_free_probes(emu_backend, monkeypatch, i, dtype):
    FL.suite_onchip_probes(emu_backend, DEV, monkeypatch, i, dtype, "emu")


@pytest.mark.parametrize("dtype", [FL.F32, FL.BF16], ids=ids)
@pytest.mark.parametrize("i", range(len(FL.D_CASES)))
def test_pitched_rows_with_guards(emu_backend, monkeypatch, i, dtype):
    FL.suite_pitched(emu_backend, DEV, monkeypatch, i, dtype, "emu")


def test_reference_against_the_direct_sum():
    """the fp64 FFT reference itself, independent of any kernel: against oracle.causal_conv_direct_f64 (no FFT) at L <= 700, the gradients
    against the same sum applied to flipped rows (corr(a, b) = flip(conv(flip a, b)))"""
    for B, D, L in ((2, 3, 1), (2, 3, 37), (1, 2, 700)):
        u, k, b, dout = FL.inputs(B, D, L, FL.F32, 5 * L)
        out, du, dk, db = FL.ref64(u, k, b, dout)
        kk, zero = k[None].expand(B, D, L).reshape(B * D, L), torch.zeros(B * D)
        want = O.causal_conv_direct_f64(u.reshape(B * D, L), kk, b.repeat(B)).view(B, D, L)
        assert float((out - want).abs().max()) < 1e-13
        want = O.causal_conv_direct_f64(dout.reshape(B * D, L).flip(-1), kk, b.repeat(B)).flip(-1).view(B, D, L)
        assert float((du - want).abs().max()) < 1e-13
        want = O.causal_conv_direct_f64(dout.reshape(B * D, L).flip(-1), u.reshape(B * D, L), zero).flip(-1).view(B, D, L).sum(0)
        assert float((dk - want).abs().max()) < 1e-13
        assert float((db - (dout.double() * u.double()).sum(dim=(0, 2))).abs().max()) == 0.0


def test_every_unreached_branch_is_named_by_a_case():
    """the kernels and host paths the suite had never run on the chip, each by the route string of at least one literal case"""
    routes = [c[-1] for c in FL.B_CASES] + [c[-1] for c in FL.C_CASES] + [FL.a_route(m) for m in FL.SUPPORTED_M1]
    for piece in ("col<192>", "col<256>", "col<320>", "col<512>", "col<128>", "col<1>", "col<28>", "row0_corr+corr", "row0_bwd<nodu>+row_bwd<nodu>",
                  "row0_bwd<nodu>+row_dk ", "chunks=1x2+1 chunks=1x2+1 saved", "conv<32,f32out>", "dk<16,2> S=1", "corr<16> dk<16,1> S=2",
                  "corr<16> dk<16,1> S=1", "dk<1,1,DU>", "dk<2,1,DU>", "dk<4,1,DU>", "dk<8,1,DU>", "S=3 ragged=1"):
        assert any(piece in r for r in routes), piece
    for R in (4, 16, 32):                                                 # du only and dk only at R > 2
        assert any(c[0] == R and c[4] == (1, 0) for c in FL.C_CASES) and any(c[0] == R and c[4] == (0, 1) for c in FL.C_CASES)
    assert any(c[0] == 32 and c[1] == 1 and FL.F16 in c[7] and c[6] is None for c in FL.C_CASES)
