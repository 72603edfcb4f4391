"""The residual glue of a block -- add_norm_fwd / add_norm_bwd (plain and embedding-gathering), the np = 3 column sums of dx0, and the pooled
readout of csrc/block_kernels.h -- on the CPU-emulated kernels, each kernel called on its own against the element-wise fp64 references and derived
bounds of tests/block_local.py: every output element within its bound, mean and rstd included, every sum within its own and its bound below its
smallest term, NaN in everything the contract does not read, a sentinel in every byte it does not write, every kernel repeatable bit for bit, the
wrappers of _lib on the same operands.  The same checks run on the gfx950 library in tests/test_gpu_block_local.py; figures of both in
profiles/block_local.md."""
import pytest
import torch
import torch.nn.functional as F

from tests import block_local as BL

DEV = torch.device("cpu")


@pytest.mark.parametrize("pair", BL.PAIRS, ids=BL.PAIR_ID.get)
@pytest.mark.parametrize("D", BL.AN_D)
def test_add_norm_kernels(emu_backend, D, pair):
    """E = 1 .. 16 at rows 1, 3, 4, 5, 37 (partial workgroups, idle wavefronts); residual, p and np cycle"""
    for case in BL.add_norm_cases(D, pair):
        BL.run_add_norm(emu_backend, DEV, label="emu", **case)


@pytest.mark.parametrize("D", [64, 128])
def test_add_norm_dropout_on_partial_philox_groups(emu_backend, D):
    """E = 1, 2: a lane holds a part of an aligned Philox group of four; p in {0, 0.1, 0.5}, with and without residual, np 2 and 3"""
    for case in BL.add_norm_dropout_cases(D):
        BL.run_add_norm(emu_backend, DEV, label="emu", **case)


@pytest.mark.parametrize("dtype", BL.DTYPES, ids=BL.NAME.get)
def test_add_norm_second_sweep(emu_backend, dtype):
    """rows = 8197 at D = 64: the grid is capped at 2048 workgroups, five rows fall into a second, partial sweep of the grid-stride loop"""
    rows, D = BL.AN_BIG
    assert BL.blk_grid(rows) == BL.BLK_MAX_GRID and rows > 4 * BL.BLK_MAX_GRID
    i = BL.DTYPES.index(dtype)
    BL.run_add_norm(emu_backend, DEV, rows, D, dtype, dtype, with_res=i != 1, p=(0.1, 0.0, 0.5)[i], np_=3 if i != 2 else 2, seed=8197 + i, label="emu")


@pytest.mark.parametrize("V", BL.EMB_V)
@pytest.mark.parametrize("D", BL.EMB_D)
def test_embed_kernels(emu_backend, D, V):
    """x0 = table[ids]: D 64 / 128 / 256, V 1 / 12 / 16, some classes empty, table rows [V, 16) NaN, d_table[V:] untouched; types and p cycle"""
    for case in BL.embed_cases(D, V):
        BL.run_embed(emu_backend, DEV, label="emu", **case)


@pytest.mark.parametrize("dtype", BL.DTYPES, ids=BL.NAME.get)
def test_embed_second_sweep(emu_backend, dtype):
    i = BL.DTYPES.index(dtype)
    BL.run_embed(emu_backend, DEV, BL.AN_BIG[0], BL.AN_BIG[1], 12, dtype, p=(0.0, 0.1, 0.5)[i], seed=8200 + i, label="emu")


@pytest.mark.parametrize("dtype", BL.DTYPES, ids=BL.NAME.get)
@pytest.mark.parametrize("rows,D,V,p", [(37, 64, 12, 0.0), (5, 128, 16, 0.1), (9, 256, 1, 0.0)])
def test_embed_backward_leaves_bad_ids_out_of_every_sum(emu_backend, rows, D, V, p, dtype):
    """ids -1 and V, `saved` as the forward leaves it (NaN rows): d_table, dweight and dbias are finite and are the sums over the remaining rows"""
    BL.run_embed_bad_ids(emu_backend, DEV, rows, D, V, dtype, p, seed=rows + D + V, label="emu")


@pytest.mark.parametrize("dtype", BL.DTYPES, ids=BL.NAME.get)
@pytest.mark.parametrize("shape", list(BL.POOL_SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_pool_kernels(emu_backend, shape, dtype):
    """both modes, lengths None and ragged (0, 1, chunk_rows - 1 .. chunk_rows + 1, L - 1, L, L + 7, -3 at B = 64), the finish kernel's unrolled
    rounds and tails, two rows per wavefront per chunk"""
    for case in BL.pool_cases(shape, dtype):
        BL.run_pool(emu_backend, DEV, label="emu", **case)


def test_lengths_hold_every_edge():
    n = BL.pool_lengths(64, 200, "ragged", DEV).tolist()
    cr = BL.pool_chunk_rows(64, 200)
    assert cr == 8 and set(n) == {0, 1, cr - 1, cr, cr + 1, 199, 200, 207, -3}
    for (B, L, D), want in BL.POOL_SHAPES.items():
        assert (BL.pool_chunk_rows(B, L), BL.pool_chunks(B, L)) == want
    assert 112 < 115 <= 115 and 128 + 112 < 258 and not 256 + 112 < 258      # the unrolled rounds of the finish kernel at 115 and 258 chunks


def test_philox_is_the_published_generator():
    """the vectorised mask generator against the scalar restatement of tests/test_block_emu.py on its first 1024 elements"""
    from tests.test_block_emu import _philox4x32_10
    got = BL.philox_words(BL.SEED, 1024, DEV).tolist()
    k0, k1 = BL.SEED & 0xFFFFFFFF, BL.SEED >> 32
    want = [w for i4 in range(256) for w in _philox4x32_10(i4, 0, k0, k1)]
    assert got == want
    assert BL.dropout_params(0.5) == (1 << 31, 2.0)


def test_references_agree_with_autograd():
    """the fp64 references themselves, independent of any kernel: the backward references are autograd's gradients of the forward references
    (dropout mask, add, F.layer_norm, masked mean / sum, F.embedding)"""
    g = torch.Generator().manual_seed(11)
    rows, D, V = 7, 64, 5
    dd = dict(generator=g, dtype=torch.float64)
    keep, ks = BL.keep_mask(0.5, (rows, D), DEV)
    w, b = torch.randn(D, **dd).requires_grad_(True), torch.randn(D, **dd).requires_grad_(True)
    eps = BL.f32(BL.EPS)
    close = lambda a_, b_: torch.allclose(a_, b_, rtol=1e-12, atol=1e-12)      # noqa: E731
    # add_norm
    x0, res = torch.randn(rows, D, **dd).requires_grad_(True), torch.randn(rows, D, **dd).requires_grad_(True)
    dout, h = torch.randn(rows, D, **dd), torch.randn(rows, D, **dd)
    r = keep * ks * x0 + res
    out = F.layer_norm(r, (D,), w, b, eps)
    R = BL.fwd64(x0, res, w, b, keep, ks)
    assert close(R["out"], out) and close(R["r"], r)
    gx, gr, gw, gb = torch.autograd.grad((out * dout).sum() + (r * h).sum(), (x0, res, w, b))
    with torch.no_grad():
        Rb = BL.bwd64(dout, R["r"], R["mean"], R["rstd"], w, h, keep, ks)
        assert close(Rb["dx"], gx) and close(Rb["dr"], gr) and close(Rb["t_dw"].sum(0), gw) and close(Rb["t_db"].sum(0), gb)
    # embedding
    table = torch.randn(V, D, **dd).requires_grad_(True)
    ids = torch.randint(0, V - 1, (rows,), generator=g)                        # class V - 1 stays empty
    r = keep * ks * F.embedding(ids, table)
    out = F.layer_norm(r, (D,), w, b, eps)
    gt, = torch.autograd.grad((out * dout).sum() + (r * h).sum(), (table,))
    with torch.no_grad():
        R = BL.fwd64(table[ids], None, w, b, keep, ks)
        Rb, onehot = BL.emb_bwd_ref(dout, R["r"], R["mean"], R["rstd"], w, h, keep, ks, ids, V)
        assert close(R["out"], out) and close(torch.einsum("rv,rd->vd", onehot, Rb["dx"]), gt) and not bool(gt[V - 1].any())
    # pooled readout
    B, L = 3, 5
    keep, ks = BL.keep_mask(0.5, (B, L, D), DEV)
    n = torch.tensor([5, 0, 2])
    x0, res = torch.randn(B, L, D, **dd).requires_grad_(True), torch.randn(B, L, D, **dd).requires_grad_(True)
    gp = torch.randn(B, D, **dd)
    for mode in ("mean", "sum"):
        out = F.layer_norm(keep * ks * x0 + res, (D,), w, b, eps)
        valid = (torch.arange(L)[None, :] < n[:, None]).double()[..., None]
        pooled = (valid * out).sum(1)
        if mode == "mean":
            pooled = pooled / n.clamp_min(1)[:, None]
        gx, gr, gw, gb = torch.autograd.grad((pooled * gp).sum(), (x0, res, w, b))
        with torch.no_grad():
            R = BL.pool_fwd64(x0, res, w, b, keep, ks, n, mode)
            Rb = BL.pool_bwd64(gp, x0, res, R["mean"], R["rstd"], w, keep, ks, n, mode)
            assert close(R["pooled"], pooled) and close(Rb["dx"], gx) and close(Rb["dr"], gr)
            assert close(Rb["t_dw"].sum((0, 1)), gw) and close(Rb["t_db"].sum((0, 1)), gb)
            assert not bool(gx[1].any()) and not bool(gx[2, 2:].any())
