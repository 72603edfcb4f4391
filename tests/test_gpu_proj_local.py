"""MI355X: the matrix-core kernels of csrc/proj_kernels.h and csrc/proj2_kernels.h -- in_proj and out_proj (both generations, out_proj also with
its LayerNorm epilogue), mlp_kernel<0> / <1>, outproj_dgrad_gate_bwd, colsum -- each kernel of the gfx950 library called on its own against the
fp64 references and derived bounds of tests/proj_local.py (evaluated by torch ops on the device): every output element within its bound, every sum
within its own and (where asserted) below the smallest single term, NaN in every gap of every input, a sentinel in every byte the contract leaves
alone, bit-equal repeats, the wrappers of _lib.  The cases and seeds are those of tests/test_proj_local_emu.py: the smallest shapes that reach each
path of the schedules (the workload shapes are tests/test_gpu_proj.py's).  Figures: profiles/proj_local.md."""
import pytest
import torch

from tests import proj_local as PL

pytestmark = pytest.mark.gpu
_ids = PL.NAME.get


def _dev():
    return torch.device("cuda", 0)


@pytest.mark.parametrize("dtype", PL.DTYPES, ids=_ids)
@pytest.mark.parametrize("gen", [1, 2])
@pytest.mark.parametrize("i", range(len(PL.INPROJ_CASES)))
def test_inproj_pre_fwd(gpu_lib, i, gen, dtype):
    PL.run_inproj(gpu_lib, _dev(), dtype, gen=gen, label="gpu", **PL.inproj_kwargs(i))


@pytest.mark.parametrize("dtype", PL.DTYPES, ids=_ids)
@pytest.mark.parametrize("P,K,N,path", PL.MLP_CASES)
def test_mlp_kernels(gpu_lib, P, K, N, path, dtype):
    PL.run_mlp(gpu_lib, _dev(), dtype, P, K, N, seed=P + N, label="gpu", path=path)


@pytest.mark.parametrize("dtype", PL.DTYPES, ids=_ids)
@pytest.mark.parametrize("gen", [1, 2])
@pytest.mark.parametrize("i", range(len(PL.OUTPROJ_CASES)))
def test_outproj_gate_fwd(gpu_lib, i, gen, dtype):
    PL.run_outproj(gpu_lib, _dev(), dtype, gen=gen, label="gpu", **PL.outproj_kwargs(i))


@pytest.mark.parametrize("dtype", PL.DTYPES, ids=_ids)
@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("i", range(len(PL.DGRAD_CASES)))
def test_outproj_dgrad_gate_bwd(gpu_lib, i, exact, dtype):
    PL.run_dgrad(gpu_lib, _dev(), dtype, exact=exact, label="gpu", **PL.dgrad_kwargs(i))


@pytest.mark.parametrize("dtype", PL.DTYPES, ids=_ids)
@pytest.mark.parametrize("P,N", PL.COLSUM_CASES)
def test_colsum(gpu_lib, P, N, dtype):
    PL.run_colsum(gpu_lib, _dev(), dtype, P, N, seed=P + N, label="gpu", path="")
