"""Sequence classification on the MI355X: the fused add + LayerNorm + pooled readout (include/hyena_block.h hyena_add_norm_pool_*) against an
fp64 graph with the unfused route (add_norm kernels + fp32 torch reduction) as the yardstick, determinism, graph capture with device-side
lengths, the fine-tuning loop of scripts/finetune_classify.py and a graphed training step of the classifier."""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pooled", "dx0", "dresidual", "dweight", "dbias")


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()


def _inputs(B, L, D, dtype, seed):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(seed)
    x0 = torch.randn(B, L, D, generator=g, device=dev).to(dtype)
    residual = torch.randn(B, L, D, generator=g, device=dev) * 2
    weight = 1 + 0.2 * torch.randn(D, generator=g, device=dev)
    bias = 0.1 * torch.randn(D, generator=g, device=dev)
    gp = torch.randn(B, D, generator=g, device=dev)
    return x0, residual, weight, bias, gp


def _run(fn, x0, residual, weight, bias, gp):
    leaves = [t.detach().clone().requires_grad_(True) for t in (x0, residual, weight, bias)]
    y = fn(*leaves)
    grads = torch.autograd.grad(y, leaves, gp.to(y.dtype))
    return [y.detach()] + [t.detach() for t in grads]


def _fp64(x0, residual, weight, bias, gp, lengths, mode):
    from hyena_dna_amd.block import masked_pool
    D = x0.shape[-1]

    def graph(x, r, w, b):
        out = torch.nn.functional.layer_norm(x + r, (D,), w, b, 1e-5)
        n = None if lengths is None else lengths
        L = out.shape[1]
        if n is None:
            s = out.sum(1)
            return s / L if mode == "mean" else s
        keep = (torch.arange(L, device=out.device).unsqueeze(0) < n.unsqueeze(1)).unsqueeze(-1)
        s = (out * keep).sum(1)
        return s / n.clamp_min(1).unsqueeze(1) if mode == "mean" else s

    return _run(graph, x0.double(), residual.double(), weight.double(), bias.double(), gp.double())


CASES = [((8, 32768, 256), "none"), ((2, 159999, 256), "ragged"), ((1, 1 << 20, 256), "none")]


@pytest.mark.parametrize("shape,kind", CASES)
def test_fused_readout_error_against_fp64_is_bounded_by_the_unfused_routes(gpu_lib, shape, kind):
    """bf16 activations.  Yardstick: |result - fp64 graph| (relative L2) of the route the code had before -- dropout_add_layer_norm (the add_norm
    kernels) followed by an fp32 torch reduction; the fused pass may be at most twice as far from fp64, value and every gradient.  (It should be
    closer: nothing is rounded to bf16 in front of the sum, and no bf16 dout exists.)  Both figures are printed, and appended to the file
    HYENA_POOL_REPORT names when it is set (profiles/pool_readout.md was written that way)."""
    from hyena_dna_amd.block import dropout_add_layer_norm, dropout_add_layer_norm_pool, masked_pool
    B, L, D = shape
    x0, residual, weight, bias, gp = _inputs(B, L, D, torch.bfloat16, seed=L % 1000 + B)
    lengths = None if kind == "none" else torch.tensor([L - 12345, 77777], device=x0.device)[:B]
    want = _fp64(x0, residual, weight, bias, gp, lengths, "mean")
    fused = _run(lambda x, r, w, b: dropout_add_layer_norm_pool(x, r, w, b, 0.0, 1e-5, lengths=lengths, mode="mean"), x0, residual, weight, bias, gp)
    unfused = _run(lambda x, r, w, b: masked_pool(dropout_add_layer_norm(x, r, w, b, 0.0, 1e-5, prenorm=False, residual_in_fp32=True), lengths, "mean"),
                   x0, residual, weight, bias, gp)
    torch.cuda.synchronize()
    rows = []
    for name, f, u, w in zip(NAMES, fused, unfused, want):
        assert f.shape == w.shape == u.shape and torch.isfinite(f.float()).all(), name
        rows.append((name, _rel(f, w), _rel(u, w)))
    print(f"\n[pool readout vs fp64] {B} x {L} x {D} bf16, lengths: {kind}")
    for name, ef, eu in rows:
        print(f"  {name:10s} fused {ef:.3e}   unfused {eu:.3e}")
    report = os.environ.get("HYENA_POOL_REPORT")
    if report:
        with open(report, "a") as f:
            for name, ef, eu in rows:
                f.write(f"| {B} x {L} x {D} | {kind} | {name} | {ef:.3e} | {eu:.3e} |\n")
    for name, ef, eu in rows:
        assert ef <= 2 * eu, (name, ef, eu)
    if lengths is not None:
        for b in range(B):
            n = int(lengths[b])
            assert not fused[1][b, n:].any() and not fused[2][b, n:].any()


def test_two_runs_are_bit_identical(gpu_lib):
    from hyena_dna_amd.block import dropout_add_layer_norm_pool
    x0, residual, weight, bias, gp = _inputs(4, 70001, 256, torch.bfloat16, seed=9)
    lengths = torch.tensor([70001, 1, 0, 33333], device=x0.device)
    torch.manual_seed(11)
    a = _run(lambda x, r, w, b: dropout_add_layer_norm_pool(x, r, w, b, 0.1, 1e-5, lengths=lengths, mode="sum"), x0, residual, weight, bias, gp)
    torch.manual_seed(11)
    b_ = _run(lambda x, r, w, b: dropout_add_layer_norm_pool(x, r, w, b, 0.1, 1e-5, lengths=lengths, mode="sum"), x0, residual, weight, bias, gp)
    for name, s, t in zip(NAMES, a, b_):
        assert torch.equal(s, t), name
    assert not a[0][2].any() and torch.isfinite(a[0]).all()


def test_one_captured_graph_serves_every_lengths_tensor(gpu_lib):
    """the launch grid depends on (B, L) only and n_b is read on the device: a graph captured with one `lengths` replays correctly with another"""
    from hyena_dna_amd.block import AddNormPoolFunc
    B, L, D = 4, 5000, 128
    x0, residual, weight, bias, gp = _inputs(B, L, D, torch.bfloat16, seed=2)
    dev = x0.device
    static_n = torch.full((B,), L, dtype=torch.int32, device=dev)
    xs, rs = x0.clone().requires_grad_(True), residual.clone().requires_grad_(True)
    ws, bs = weight.clone().requires_grad_(True), bias.clone().requires_grad_(True)

    def step():
        y = AddNormPoolFunc.apply(xs, rs, ws, bs, 1e-5, static_n, "mean")
        return [y] + list(torch.autograd.grad(y, [xs, rs, ws, bs], gp))

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            outs = step()
    torch.cuda.current_stream(dev).wait_stream(side)
    for n in ([L, 1, 2500, 0], [17, L - 1, L, 4097]):
        static_n.copy_(torch.tensor(n, dtype=torch.int32, device=dev))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in outs]
        eager = step()
        torch.cuda.synchronize()
        for name, s, t in zip(NAMES, replayed, eager):
            assert torch.equal(s, t), (name, n)


def _script():
    spec = importlib.util.spec_from_file_location("finetune_classify", os.path.join(ROOT, "scripts", "finetune_classify.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


FINETUNE_STEPS = 1500


@pytest.mark.parametrize("fused", [True, False])
def test_finetune_loop_learns_the_planted_motif(gpu_lib, fused):
    """scripts/finetune_classify.py's loop: 2 layers, d_model 128, L <= 128, bf16 autocast, END-padded variable-length batches,
    the motif planted four times in the positive class.  The loss after
    training is below the loss at step 0 and the held-out accuracy is above the majority-class rate.  FINETUNE_STEPS was chosen so that the
    UNFUSED route (final norm over all positions + fp32 reduction: the second parameter value, same seeds) reaches both as well: at 1500
    steps both routes are at loss < 0.01 and held-out accuracy > 0.99 (400 steps at lr 2e-3 left either at ln 2)."""
    from hyena_dna_amd.runner import make_synthetic_classification
    ft = _script()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = ft.build_classifier(d_model=128, n_layer=2, max_length=128, fused_readout=fused).to(dev)
    ids, _, labels = make_synthetic_classification(2048, 128, seed=0, copies=4)
    h_ids, _, h_labels = make_synthetic_classification(512, 128, seed=1, copies=4)
    out = ft.finetune(model, (ids.to(dev), labels.to(dev)), (h_ids.to(dev), h_labels.to(dev)), FINETUNE_STEPS, batch_size=32, lr=1e-3)
    print(f"\n[finetune fused={fused}] {out}")
    assert out["last_loss"] < out["first_loss"], out
    assert out["accuracy"] > out["majority"], out


def test_graphed_train_step_on_the_classifier_matches_an_eager_step(gpu_lib):
    """lm.GraphedTrainStep calls model.loss(ids, targets, ignore_index=...) with labels of shape (B,): one captured step == one eager step from the
    same state (loss and every parameter after the update)"""
    import copy
    from hyena_dna_amd.lm import GraphedTrainStep
    from hyena_dna_amd.runner import make_synthetic_classification
    ft = _script()
    dev = torch.device("cuda", 0)
    torch.manual_seed(3)
    model = ft.build_classifier(d_model=128, n_layer=2, max_length=256, embed_dropout=0.0).to(dev)
    twin = copy.deepcopy(model)
    ids, _, labels = make_synthetic_classification(16, 256, seed=5)
    ids, labels = ids.to(dev), labels.to(dev)
    ids2, _, labels2 = make_synthetic_classification(16, 256, seed=6)
    ids2, labels2 = ids2.to(dev), labels2.to(dev)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.1, capturable=True)
    step = GraphedTrainStep(model, opt, ids, labels)
    loss_g = step(ids2, labels2).item()                       # another batch, other lengths: the same graph
    opt_t = torch.optim.AdamW(twin.parameters(), lr=1e-3, weight_decay=0.1, capturable=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss_e = twin.loss(ids2, labels2)
    loss_e.backward()
    opt_t.step()
    torch.cuda.synchronize()
    # the bounds tests/test_gpu_block.py holds the language model's graphed step to (same kernels in the same order on both sides)
    assert abs(loss_g - loss_e.item()) <= 2e-3 * abs(loss_e.item()), (loss_g, loss_e.item())
    for (name, p), q in zip(model.named_parameters(), twin.parameters()):
        assert torch.allclose(p, q, rtol=2e-2, atol=2e-4), name
    step.release()
