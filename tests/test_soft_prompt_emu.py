"""Soft-prompt tuning on the CPU-emulated kernels: soft_embed_add_norm_fwd / _bwd of csrc/block_kernels.h, each called on its own through the C ABI against
the fp64 references and bounds of tests/soft_prompt_local.py, the bit-exact cross-checks against add_norm_fwd / add_norm_bwd, bad ids, and the model
level (HyenaDNALM's soft-token route, hidden_at, soft_prompt.SoftPromptLM); host only: the few-shot dataset layout and the label positions.  The same
kernel and model cases run on the gfx950 library in tests/test_gpu_soft_prompt.py."""
import pytest
import torch

from tests import soft_prompt_local as SP

DEV = lambda: torch.device("cpu")      # noqa: E731
LABEL = "emu"


@pytest.mark.parametrize("V", SP.SOFT_V)
@pytest.mark.parametrize("D", SP.SOFT_D)
def test_soft_kernels(emu_backend, D, V):
    """(B, n, L) = (1,1,1), (2,3,7), (3,4,1), (2,5,3), (3,37,2) at every (D, V); types, both dropouts and d_residual_out cycle"""
    for case in SP.soft_cases(D, V):
        SP.run_soft(emu_backend, DEV(), label=LABEL, **case)


@pytest.mark.parametrize("case", list(SP.big_cases()), ids=["fwd-3x2050x700", "bwd-1x8197x1"])
def test_soft_kernels_second_sweep(emu_backend, case):
    """forward: 8250 rows, above the 2048 x 4 rows of one grid sweep; backward: 8197 soft positions"""
    B, n, L = case["B"], case["n"], case["L"]
    assert SP.BL.blk_grid(B * (n + L)) == SP.BL.BLK_MAX_GRID and max(B * (n + L), n) > 4 * SP.BL.BLK_MAX_GRID
    SP.run_soft(emu_backend, DEV(), label=LABEL, wrappers=False, **case)


@pytest.mark.parametrize("D", SP.SOFT_D)
def test_forward_is_add_norm_fwd_on_the_concatenation_bit_for_bit(emu_backend, D):
    for k, (B, n, L) in enumerate(SP.SOFT_SHAPES):
        SP.run_cross_check_fwd(emu_backend, DEV(), B, n, L, D, SP.SOFT_V[(k + D // 64) % 3], SP.DTYPES[(k + D // 128) % 3], (0.0, 0.1)[k % 2], seed=D + k)


@pytest.mark.parametrize("D", SP.SOFT_D)
def test_backward_is_the_sum_of_add_norm_bwd_soft_rows_bit_for_bit(emu_backend, D):
    for k, (B, n, L) in enumerate([(1, 1, 1), (2, 3, 7), (1, 4, 1), (2, 5, 3), (2, 37, 2), (1, 37, 2)]):
        SP.run_cross_check_bwd(emu_backend, DEV(), B, n, L, D, SP.DTYPES[(k + D // 128) % 3], (0.1, 0.0)[k % 2], with_h=bool((k // 2) % 2), seed=7 * D + k)


@pytest.mark.parametrize("D,V,p,sp", [(64, 12, 0.0, 0.0), (128, 16, 0.1, 0.5), (256, 1, 0.1, 0.0)])
def test_bad_ids_poison_their_own_rows_only(emu_backend, D, V, p, sp):
    for k, OT in enumerate(SP.DTYPES):
        SP.run_bad_ids(emu_backend, DEV(), 2, 3, 5, D, V, OT, p, sp, seed=D + V + k)


def test_bad_arguments_are_refused_before_any_launch(emu_backend):
    SP.check_bad_args(emu_backend, DEV())


@pytest.mark.parametrize("B,n,L", SP.MODEL_CASES)
def test_model_fused_route_equals_unfused_route_fp32(emu_backend, B, n, L):
    SP.check_fused_equals_unfused_fp32(DEV(), B, n, L)


@pytest.mark.parametrize("V", SP.SOFT_V)
@pytest.mark.parametrize("D", SP.SOFT_D)
def test_row_head_kernels(emu_backend, D, V):
    """the row-wise head, forward and backward: fp64 bounds, guards, repeatable, a row's logits independent of the other rows of the call"""
    for k, rows in enumerate(SP.HEAD_ROWS):
        SP.run_row_head(emu_backend, DEV(), rows, D, V, SP.DTYPES[(k + D // 64 + SP.SOFT_V.index(V)) % 3], seed=D + V + rows, label=LABEL)


def test_row_head_autograd_and_fallback(emu_backend):
    SP.check_row_head_autograd(DEV())


@pytest.mark.parametrize("B,n,L", SP.MODEL_CASES)
def test_model_hidden_at_gives_the_rows_of_the_full_final_norm(emu_backend, B, n, L):
    SP.check_hidden_at_rows(DEV(), B, n, L)


@pytest.mark.parametrize("B,n,L", SP.MODEL_CASES)
def test_model_hidden_at_plus_head_equals_the_rows_of_the_full_logits_bit_for_bit(emu_backend, B, n, L):
    SP.check_hidden_at_plus_head_bit_for_bit(DEV(), B, n, L)


# (bf16 autocast runs on the device only, tests/test_gpu_soft_prompt.py: the package's Mlp / projection / filter paths read the device autocast state,
# so under CPU autocast on the emulator they would stay fp32 while the new first norm hands them bf16)


def test_model_dropouts_repeat_from_the_seed_and_soft_mask_is_shared_by_the_batch(emu_backend):
    SP.check_dropouts_repeat(DEV())


def test_model_tuning_lowers_the_loss_and_moves_only_the_prompt(emu_backend):
    SP.check_tuning_moves_only_the_prompt(DEV())


def test_model_limits_and_plain_model(emu_backend):
    SP.check_limits_and_plain_model(DEV())


def test_model_padding_of_an_odd_total(emu_backend, monkeypatch):
    SP.check_padding(DEV(), monkeypatch)


def test_references_alone_keep_every_sum_bound_below_its_smallest_term():
    """no kernel: for every case of the kernel tests the bound of d_soft stays below the smallest non-zero term of the same sum"""
    for case in SP.all_cases():
        m = SP.reference_margin(**case)
        assert m < 1.0, (case, m)


def test_backward_reference_is_autograd_of_the_forward_reference():
    """the fp64 statement itself: d_soft of the references = autograd's gradient of LayerNorm(dropout(cat([softdrop(soft), table[ids]])))"""
    import torch.nn.functional as F
    B, n, L, D, V, p, sp = 3, 4, 2, 64, 5, 0.1, 0.5
    g = torch.Generator().manual_seed(1)
    dd = dict(generator=g, dtype=torch.float64)
    dev = torch.device("cpu")
    soft, table = torch.randn(n, D, **dd).requires_grad_(True), torch.randn(V, D, **dd)
    w, b = torch.randn(D, **dd), torch.randn(D, **dd)
    ids = torch.randint(0, V, (B, L), generator=g)
    keep, ks = SP.keep_mask(p, (B, n + L, D), dev)
    keep2, ks2 = SP.soft_keep(sp, n, D, dev)
    r = keep * ks * torch.cat([(keep2 * ks2 * soft).unsqueeze(0).expand(B, n, D), table[ids]], 1)
    out = F.layer_norm(r, (D,), w, b, SP.f32(SP.EPS))
    dout, h = torch.randn(B, n + L, D, **dd), torch.randn(B, n + L, D, **dd)
    want, = torch.autograd.grad((out * dout).sum() + (r * h).sum(), (soft,))
    with torch.no_grad():
        R = SP.fwd64(r / 1.0, None, w, b, None, 1.0)
        Rb = SP.bwd64(dout[:, :n].reshape(B * n, D), R["r"][:, :n].reshape(B * n, D), R["mean"][:, :n].reshape(-1), R["rstd"][:, :n].reshape(-1), w,
                      h[:, :n].reshape(B * n, D), keep[:, :n].reshape(B * n, D), ks)
        got = keep2 * ks2 * Rb["dx"].view(B, n, D).sum(0)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("shots", [0, 1, 2])
def test_few_shot_dataset_layout_and_label_positions(shots):
    import numpy as np
    from hyena_dna_amd import ICLFewShotDataset, few_shot_label_positions
    from hyena_dna_amd.tokenizer import DNACharTokenizerLUT
    M = 6
    rng = np.random.RandomState(0)
    seqs = ["".join(rng.choice(list("ACGT"), M)) for _ in range(10)]
    labels = [i % 2 for i in range(10)]
    tok = DNACharTokenizerLUT()
    ds = ICLFewShotDataset(seqs, labels, shots, M, tokenizer=tok, label_to_token={0: "A", 1: "N"})
    assert len(ds) == 10
    name = {0: tok.vocab["A"], 1: tok.vocab["N"]}
    enc = {tuple(tok.vocab[c] for c in s): y for s, y in zip(seqs, labels)}
    np.random.seed(3)
    orders = set()
    for idx in range(10):
        x, y = ds[idx]
        assert x.dtype == torch.int64 and y.shape == (1,) and y.item() == name[labels[idx]]
        assert x.shape == (2 * shots * (M + 3) + M + 1,)
        assert x[-M - 1:].tolist() == [tok.vocab[c] for c in seqs[idx]] + [tok.sep_token_id]
        seen = []
        for k in range(2 * shots):                            # every shot: seq + eos + label + eos, the label its own sequence's
            blk = x[k * (M + 3):(k + 1) * (M + 3)].tolist()
            assert blk[M] == tok.sep_token_id and blk[M + 2] == tok.sep_token_id
            assert tuple(blk[:M]) in enc and blk[M + 1] == name[enc[tuple(blk[:M])]] and blk[:M] != x[-M - 1:-1].tolist()
            seen.append(enc[tuple(blk[:M])])
        assert sorted(seen) == [0] * shots + [1] * shots      # `shots` per class
        orders.add(tuple(seen))
        full = torch.cat([x, y])
        pos = few_shot_label_positions(M, full.shape[0])
        formula = [M + 1] + list(range(2 * M + 4, full.shape[0], M + 3))
        assert pos.tolist() == formula
        if shots > 0:                                         # the formula counts one label per (max_length + 3)-token shot, then the test label
            actual = [k * (M + 3) + M + 1 for k in range(2 * shots)] + [full.shape[0] - 1]
            assert pos.tolist() == actual
            assert all(int(full[q]) in name.values() for q in pos)
    if shots > 0:
        assert len(orders) > 1                                # the shots are shuffled
    short = ICLFewShotDataset(["ACGTACGTAC", "AC"], [0, 1], 0, 4, add_eos=False)
    assert short[0][0].tolist() == [7, 8, 9, 10] and short[1][0].tolist() == [7, 8] and short[1][1].tolist() == [tok.vocab["N"]]
    with pytest.raises(ValueError):
        ICLFewShotDataset(["AC", "GT"], [0, 1], 1, 4)
