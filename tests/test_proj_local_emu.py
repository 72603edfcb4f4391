"""The matrix-core kernels of csrc/proj_kernels.h and csrc/proj2_kernels.h -- in_proj and out_proj (both generations, out_proj also with its
LayerNorm epilogue), mlp_kernel<0> / <1>, outproj_dgrad_gate_bwd, colsum -- on the CPU-emulated kernels, each called on its own against the fp64
references and derived bounds of tests/proj_local.py: every output element within its bound, every sum within its own and (where asserted) below
the smallest single term, NaN in every gap of every input, a sentinel in every byte the contract leaves alone, bit-equal repeats, the wrappers of
_lib.  The same cases run on the gfx950 library in tests/test_gpu_proj_local.py; figures of both in profiles/proj_local.md."""
import pytest
import torch

from tests import proj_local as PL

DEV = torch.device("cpu")
_ids = PL.NAME.get


@pytest.mark.parametrize("dtype", PL.DTYPES, ids=_ids)
@pytest.mark.parametrize("gen", [1, 2])
@pytest.mark.parametrize("i", range(len(PL.INPROJ_CASES)))
def test_inproj_pre_fwd(emu_backend, i, gen, dtype):
    PL.run_inproj(emu_backend, DEV, dtype, gen=gen, label="emu", **PL.inproj_kwargs(i))


@pytest.mark.parametrize("dtype", PL.DTYPES, ids=_ids)
@pytest.mark.parametrize("P,K,N,path", PL.MLP_CASES)
def test_mlp_kernels(emu_backend, P, K, N, path, dtype):
    PL.run_mlp(emu_backend, DEV, dtype, P, K, N, seed=P + N, label="emu", path=path)


@pytest.mark.parametrize("dtype", PL.DTYPES, ids=_ids)
@pytest.mark.parametrize("gen", [1, 2])
@pytest.mark.parametrize("i", range(len(PL.OUTPROJ_CASES)))
def test_outproj_gate_fwd(emu_backend, i, gen, dtype):
    PL.run_outproj(emu_backend, DEV, dtype, gen=gen, label="emu", **PL.outproj_kwargs(i))


@pytest.mark.parametrize("dtype", PL.DTYPES, ids=_ids)
@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("i", range(len(PL.DGRAD_CASES)))
def test_outproj_dgrad_gate_bwd(emu_backend, i, exact, dtype):
    PL.run_dgrad(emu_backend, DEV, dtype, exact=exact, label="emu", **PL.dgrad_kwargs(i))


@pytest.mark.parametrize("dtype", PL.DTYPES, ids=_ids)
@pytest.mark.parametrize("P,N", PL.COLSUM_CASES)
def test_colsum(emu_backend, P, N, dtype):
    PL.run_colsum(emu_backend, DEV, dtype, P, N, seed=P + N, label="emu", path="")


@pytest.mark.parametrize("B,L", [(1, 1 << 20), (1, (1 << 20) - 1), (8, 32767), (2, 159999), (1, 1000000)])
def test_schedule_at_the_workload_sizes(emu_backend, B, L):
    """the small cases above never reach the cap on runs (2^20 positions: 16384 tiles on 512 - 1024 runs): the partial buffers of mlp_kernel<1> and
    the dgrad kernel at the workload's position counts against PL.schedule (size queries: nothing is launched)"""
    lib = emu_backend.lib()
    for N in (512, 1024):
        runs, tpw = PL.mlp_schedule(B * L, N)
        assert lib.hyena_mlp_partial_floats(B * L, N) == runs * N, (B, L, N)
    for D in (128, 256):
        runs, tpw = PL.dgrad_schedule(B, L, D)
        assert lib.hyena_outproj_dgrad_partial_floats(B, L, D) == D * runs * 8, (B, L, D)


def test_references_alone():
    """the references and bounds without any kernel: the GELU derivative is autograd's, its error model covers an fp32 evaluation of pm_gelu's
    operation order, and the operands drawn for the cases keep the bound of a product below its smallest term in fp16"""
    x = torch.linspace(-9.0, 9.0, 20001, dtype=torch.float64, requires_grad=True)
    (gx,) = torch.autograd.grad(PL.gelu64(x).sum(), x)
    ref = torch.nn.functional.gelu(x.detach(), approximate="tanh")
    with torch.no_grad():
        assert torch.allclose(gx, PL.dgelu64(x), rtol=1e-12, atol=1e-14) and torch.allclose(PL.gelu64(x), ref, rtol=1e-12, atol=1e-14)
        xf = x.float()
        e = torch.exp2(xf * torch.addcmul(torch.tensor(-2.302208198), xf * xf, torch.tensor(-0.1029432396)))
        sg = 1.0 / (1.0 + e)
        assert bool(((xf * sg).double() - PL.gelu64(xf.double())).abs().le(PL.gelu_err(xf.double())).all())
        q = xf * torch.addcmul(torch.tensor(1.5957691216), xf * xf, torch.tensor(0.2140644488))
        got = torch.addcmul(sg, q * sg, 1.0 - sg)
        assert bool((got.double() - PL.dgelu64(xf.double())).abs().le(PL.dgelu_err(xf.double())).all())
    g = torch.Generator().manual_seed(1)
    for T in PL.DTYPES:
        W, u = PL._op((64, 256), g, T, DEV, PL.W_SCALE).double(), PL._op((500, 256), g, T, DEV).double()
        s, E = PL.product64(W, u)
        margin = float((E + PL.half_ulp_io(s.abs() + E, T)).max()) / (float(W.abs().min()) * float(u.abs().min()))
        assert margin < 1.0 or T == torch.bfloat16, (T, margin)
