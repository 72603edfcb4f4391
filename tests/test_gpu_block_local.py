"""MI355X: the residual glue of a block -- add_norm_fwd / add_norm_bwd (plain and embedding-gathering), the np = 3 column sums of dx0, and the
pooled readout of csrc/block_kernels.h -- each kernel of the gfx950 library called on its own against the element-wise fp64 references and derived
bounds of tests/block_local.py (evaluated by torch ops on the device).  The cases are those of tests/test_block_local_emu.py: the smallest shapes
that reach each code path.  Figures: profiles/block_local.md."""
import pytest
import torch

from tests import block_local as BL

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


@pytest.mark.parametrize("pair", BL.PAIRS, ids=BL.PAIR_ID.get)
@pytest.mark.parametrize("D", BL.AN_D)
def test_add_norm_kernels(gpu_lib, D, pair):
    """E = 1 .. 16 at rows 1, 3, 4, 5, 37 (partial workgroups, idle wavefronts); residual, p and np cycle"""
    for case in BL.add_norm_cases(D, pair):
        BL.run_add_norm(gpu_lib, _dev(), label="gpu", **case)


@pytest.mark.parametrize("D", [64, 128])
def test_add_norm_dropout_on_partial_philox_groups(gpu_lib, D):
    """E = 1, 2: a lane holds a part of an aligned Philox group of four; p in {0, 0.1, 0.5}, with and without residual, np 2 and 3"""
    for case in BL.add_norm_dropout_cases(D):
        BL.run_add_norm(gpu_lib, _dev(), label="gpu", **case)


@pytest.mark.parametrize("dtype", BL.DTYPES, ids=BL.NAME.get)
def test_add_norm_second_sweep(gpu_lib, dtype):
    """rows = 8197 at D = 64: the grid is capped at 2048 workgroups, five rows fall into a second, partial sweep of the grid-stride loop"""
    rows, D = BL.AN_BIG
    i = BL.DTYPES.index(dtype)
    BL.run_add_norm(gpu_lib, _dev(), rows, D, dtype, dtype, with_res=i != 1, p=(0.1, 0.0, 0.5)[i], np_=3 if i != 2 else 2, seed=8197 + i, label="gpu")


@pytest.mark.parametrize("V", BL.EMB_V)
@pytest.mark.parametrize("D", BL.EMB_D)
def test_embed_kernels(gpu_lib, D, V):
    """x0 = table[ids]: D 64 / 128 / 256, V 1 / 12 / 16, some classes empty, table rows [V, 16) NaN, d_table[V:] untouched; types and p cycle"""
    for case in BL.embed_cases(D, V):
        BL.run_embed(gpu_lib, _dev(), label="gpu", **case)


@pytest.mark.parametrize("dtype", BL.DTYPES, ids=BL.NAME.get)
def test_embed_second_sweep(gpu_lib, dtype):
    i = BL.DTYPES.index(dtype)
    BL.run_embed(gpu_lib, _dev(), BL.AN_BIG[0], BL.AN_BIG[1], 12, dtype, p=(0.0, 0.1, 0.5)[i], seed=8200 + i, label="gpu")


@pytest.mark.parametrize("dtype", BL.DTYPES, ids=BL.NAME.get)
@pytest.mark.parametrize("rows,D,V,p", [(37, 64, 12, 0.0), (5, 128, 16, 0.1), (9, 256, 1, 0.0)])
def test_embed_backward_leaves_bad_ids_out_of_every_sum(gpu_lib, rows, D, V, p, dtype):
    """ids -1 and V, `saved` as the forward leaves it (NaN rows): d_table, dweight and dbias are finite and are the sums over the remaining rows"""
    BL.run_embed_bad_ids(gpu_lib, _dev(), rows, D, V, dtype, p, seed=rows + D + V, label="gpu")


@pytest.mark.parametrize("dtype", BL.DTYPES, ids=BL.NAME.get)
@pytest.mark.parametrize("shape", list(BL.POOL_SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_pool_kernels(gpu_lib, shape, dtype):
    """both modes, lengths None and ragged (0, 1, chunk_rows - 1 .. chunk_rows + 1, L - 1, L, L + 7, -3 at B = 64), the finish kernel's unrolled
    rounds and tails, two rows per wavefront per chunk"""
    for case in BL.pool_cases(shape, dtype):
        BL.run_pool(gpu_lib, _dev(), label="gpu", **case)
