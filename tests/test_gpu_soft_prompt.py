"""MI355X: the soft-prompt forms of the first block's norm (soft_embed_add_norm_fwd / _bwd of the gfx950 library) and the model-level soft-token route,
on the cases of tests/test_soft_prompt_emu.py: references, bounds and checks in tests/soft_prompt_local.py."""
import pytest
import torch

from tests import soft_prompt_local as SP

pytestmark = pytest.mark.gpu
DEV = lambda: torch.device("cuda", 0)      # noqa: E731
LABEL = "gpu"


@pytest.mark.parametrize("V", SP.SOFT_V)
@pytest.mark.parametrize("D", SP.SOFT_D)
def test_soft_kernels(gpu_lib, D, V):
    """(B, n, L) = (1,1,1), (2,3,7), (3,4,1), (2,5,3), (3,37,2) at every (D, V); types, both dropouts and d_residual_out cycle"""
    for case in SP.soft_cases(D, V):
        SP.run_soft(gpu_lib, DEV(), label=LABEL, **case)


@pytest.mark.parametrize("case", list(SP.big_cases()), ids=["fwd-3x2050x700", "bwd-1x8197x1"])
def test_soft_kernels_second_sweep(gpu_lib, case):
    """forward: 8250 rows, above the 2048 x 4 rows of one grid sweep; backward: 8197 soft positions"""
    B, n, L = case["B"], case["n"], case["L"]
    assert SP.BL.blk_grid(B * (n + L)) == SP.BL.BLK_MAX_GRID and max(B * (n + L), n) > 4 * SP.BL.BLK_MAX_GRID
    SP.run_soft(gpu_lib, DEV(), label=LABEL, wrappers=False, **case)


@pytest.mark.parametrize("D", SP.SOFT_D)
def test_forward_is_add_norm_fwd_on_the_concatenation_bit_for_bit(gpu_lib, D):
    for k, (B, n, L) in enumerate(SP.SOFT_SHAPES):
        SP.run_cross_check_fwd(gpu_lib, DEV(), B, n, L, D, SP.SOFT_V[(k + D // 64) % 3], SP.DTYPES[(k + D // 128) % 3], (0.0, 0.1)[k % 2], seed=D + k)


@pytest.mark.parametrize("D", SP.SOFT_D)
def test_backward_is_the_sum_of_add_norm_bwd_soft_rows_bit_for_bit(gpu_lib, D):
    for k, (B, n, L) in enumerate([(1, 1, 1), (2, 3, 7), (1, 4, 1), (2, 5, 3), (2, 37, 2), (1, 37, 2)]):
        SP.run_cross_check_bwd(gpu_lib, DEV(), B, n, L, D, SP.DTYPES[(k + D // 128) % 3], (0.1, 0.0)[k % 2], with_h=bool((k // 2) % 2), seed=7 * D + k)


@pytest.mark.parametrize("D,V,p,sp", [(64, 12, 0.0, 0.0), (128, 16, 0.1, 0.5), (256, 1, 0.1, 0.0)])
def test_bad_ids_poison_their_own_rows_only(gpu_lib, D, V, p, sp):
    for k, OT in enumerate(SP.DTYPES):
        SP.run_bad_ids(gpu_lib, DEV(), 2, 3, 5, D, V, OT, p, sp, seed=D + V + k)


def test_bad_arguments_are_refused_before_any_launch(gpu_lib):
    SP.check_bad_args(gpu_lib, DEV())


@pytest.mark.parametrize("B,n,L", SP.MODEL_CASES)
def test_model_fused_route_equals_unfused_route_fp32(gpu_lib, B, n, L):
    SP.check_fused_equals_unfused_fp32(DEV(), B, n, L)


@pytest.mark.parametrize("V", SP.SOFT_V)
@pytest.mark.parametrize("D", SP.SOFT_D)
def test_row_head_kernels(gpu_lib, D, V):
    """the row-wise head, forward and backward: fp64 bounds, guards, repeatable, a row's logits independent of the other rows of the call"""
    for k, rows in enumerate(SP.HEAD_ROWS):
        SP.run_row_head(gpu_lib, DEV(), rows, D, V, SP.DTYPES[(k + D // 64 + SP.SOFT_V.index(V)) % 3], seed=D + V + rows, label=LABEL)


def test_row_head_autograd_and_fallback(gpu_lib):
    SP.check_row_head_autograd(DEV())


@pytest.mark.parametrize("B,n,L", SP.MODEL_CASES)
def test_model_hidden_at_gives_the_rows_of_the_full_final_norm(gpu_lib, B, n, L):
    SP.check_hidden_at_rows(DEV(), B, n, L)


@pytest.mark.parametrize("B,n,L", SP.MODEL_CASES)
def test_model_hidden_at_plus_head_equals_the_rows_of_the_full_logits_bit_for_bit(gpu_lib, B, n, L):
    SP.check_hidden_at_plus_head_bit_for_bit(DEV(), B, n, L)


@pytest.mark.parametrize("B,n,L", [(2, 5, 59), (1, 1, 122)])
def test_model_fused_route_under_bf16_autocast(gpu_lib, B, n, L):
    SP.check_autocast(DEV(), B, n, L)


def test_model_dropouts_repeat_from_the_seed_and_soft_mask_is_shared_by_the_batch(gpu_lib):
    SP.check_dropouts_repeat(DEV())


def test_model_tuning_lowers_the_loss_and_moves_only_the_prompt(gpu_lib):
    SP.check_tuning_moves_only_the_prompt(DEV())


def test_model_limits_and_plain_model(gpu_lib):
    SP.check_limits_and_plain_model(DEV())


def test_model_padding_of_an_odd_total(gpu_lib, monkeypatch):
    SP.check_padding(DEV(), monkeypatch)
