"""MI355X: the autograd layer (the 17 torch.autograd.Functions of hyena_dna_amd) on the gfx950 library -- the suites of
tests/test_autograd_local_emu.py (registry sweep, no_grad forward, gradient layouts, retained graphs, checkpointed and frozen language models,
the _gradsum side table) on the device, every Function entered through the wrapper that selects it, plus the routes only the device takes:
out_proj's fused input gradient under the auto policy, the two-level plan with and without kept spectra, the filter on its second stream,
``hyena_linear`` / ``small_vocab_embedding`` through their row-count gates, and dropout seeds under hipGraph replay.  Reads nothing outside the
repository.  Tables, counts and run times: profiles/autograd_local.md."""
import pytest
import torch

from tests import autograd_local as AL

pytestmark = pytest.mark.gpu

_CASES = [(key, i) for key, e in AL.REGISTRY.items() for i in range(len(e.cases(True)))]
_case_ids = [f"{k}-c{i}" for k, i in _CASES]
_MIXER_CASES = [(k, i) for k, i in _CASES if k in AL.MIXERS]


def _dev():
    return torch.device("cuda", 0)


@pytest.mark.parametrize("key,i,name", [p[:3] for p in AL.sweep_params(True)], ids=[p[3] for p in AL.sweep_params(True)])
def test_freeze_pattern(gpu_lib, key, i, name):
    AL.suite_pattern(gpu_lib, _dev(), key, i, name, gpu=True)


@pytest.mark.parametrize("key,i", _CASES, ids=_case_ids)
def test_forward_under_no_grad(gpu_lib, key, i):
    AL.suite_no_grad(gpu_lib, _dev(), key, i, gpu=True)


@pytest.mark.parametrize("key,i", _CASES, ids=_case_ids)
def test_gradient_layouts(gpu_lib, key, i):
    AL.suite_layouts(gpu_lib, _dev(), key, i, gpu=True)


@pytest.mark.parametrize("key,i", _MIXER_CASES, ids=[f"{k}-c{i}" for k, i in _MIXER_CASES])
def test_retained_graph(gpu_lib, monkeypatch, key, i):
    AL.suite_retained(gpu_lib, _dev(), key, i, gpu=True, mp=monkeypatch)


@pytest.mark.parametrize("saved", [True, False], ids=["saved[spectra=absent]", "recompute"])
@pytest.mark.parametrize("key", list(AL.TWO_LEVEL))
def test_retained_graph_two_level(gpu_lib, monkeypatch, key, saved):
    """L = 3069 on the two-level plan, with the forward's spectra kept (they hold the input's transform: the first backward reads no input, the
    second recomputes everything) and without"""
    how = AL.suite_retained_two_level(gpu_lib, _dev(), monkeypatch, key, saved)
    assert how.startswith("spectra=absent") == saved


def test_fused_out_proj_input_gradient_is_taken_by_the_auto_policy(gpu_lib):
    """(2, 127, 256) bf16: mixer._dgrad_fused says yes without any knob, and the backward runs outproj_dgrad_gate_bwd instead of the library GEMM +
    cm_post_bwd; (2, 127, 128) stays on the pair"""
    import hyena_dna_amd.mixer as MX
    assert MX.DGRAD_MFMA == "auto"
    key = "HyenaMixerOutCMFunc"
    labels = {}
    for i in range(len(AL.REGISTRY[key].cases(True))):
        case, base = AL.case_and_base(gpu_lib, _dev(), key, i, True)
        labels[case.label] = base.spies.kernels()
    fused = labels["mixer_out-bf16-B2-L127-D256"]
    assert "outproj_dgrad_gate_bwd" in fused and "cm_post_bwd" not in fused, fused
    pair = labels["mixer_out-bf16-B2-L127-D128"]
    assert "outproj_dgrad_gate_bwd" not in pair and "cm_post_bwd" in pair, pair


def test_gated_functions_are_entered_through_their_gates(gpu_lib):
    """hyena_linear on 32769 rows and small_vocab_embedding on 32769 ids: SplitKLinearFunc / SmallVocabEmbeddingFunc run (Case.call goes through the
    public wrappers on the device; run() asserts the spy on ``apply``), and one row fewer than the gate stays on the library path"""
    from hyena_dna_amd.projection import MIN_ROWS, hyena_linear
    assert MIN_ROWS == 32768
    for key in ("SplitKLinearFunc", "SmallVocabEmbeddingFunc"):
        for i in range(len(AL.REGISTRY[key].cases(True))):
            case, base = AL.case_and_base(gpu_lib, _dev(), key, i, True)
            assert base.spies.ran[key] == 1 and "32769" in case.label
    x = torch.randn(MIN_ROWS - 1, 64, device=_dev(), requires_grad=True)
    w = torch.randn(64, 64, device=_dev(), requires_grad=True)
    with AL.Spies(gpu_lib) as sp:
        hyena_linear(x, w, None).sum().backward()
    assert not sp.ran


_LM = [(cfg, ck) for cfg in AL.LM_GRID for ck in AL.CKPT]


@pytest.mark.parametrize("cfg,ck", _LM, ids=[AL.lm_id(*c) + f"-mixer{int(k[0])}-mlp{int(k[1])}" for c, k in _LM])
def test_lm_checkpointing(gpu_lib, cfg, ck):
    AL.suite_lm_checkpoint(gpu_lib, _dev(), cfg, ck)


_LMF = [(cfg, ck, f) for cfg in AL.LM_CROSS for ck in AL.CKPT for f in ("biases_only", "filter_only")]


@pytest.mark.parametrize("cfg,ck,freeze", _LMF, ids=[AL.lm_id(*c) + f"-mixer{int(k[0])}-mlp{int(k[1])}-{f}" for c, k, f in _LMF])
def test_lm_checkpointing_under_freezing(gpu_lib, cfg, ck, freeze):
    AL.suite_lm_checkpoint(gpu_lib, _dev(), cfg, ck, freeze)


_LMG = [(cfg, ck, f) for cfg in AL.LM_CROSS for ck in [(False, False), (True, True)] for f in ("out_proj_bias_only", "fc2_bias_only")]


@pytest.mark.parametrize("cfg,ck,freeze", _LMG, ids=[AL.lm_id(*c) + f"-mixer{int(k[0])}-mlp{int(k[1])}-{f}" for c, k, f in _LMG])
def test_lm_bias_only_with_and_without_the_side_table(gpu_lib, cfg, ck, freeze):
    AL.suite_lm_gradsum(gpu_lib, _dev(), cfg, ck, freeze)


def test_lm_autocast_reaches_the_matrix_core_functions(gpu_lib):
    """under device autocast at d_model 128 the model runs InProjPreCMFunc and FusedMlpFunc (the emulator's host autocast does not reach them
    through the model), and checkpointing recomputes them"""
    ref = AL.lm_run(gpu_lib, _dev(), (128, AL.BF16, 2, 0.1))
    got = AL.lm_run(gpu_lib, _dev(), (128, AL.BF16, 2, 0.1), (True, True))
    for f in ("InProjPreCMFunc", "FusedMlpFunc", "HyenaFilterFunc"):
        assert ref["ran"].get(f, 0) >= 2 and got["ran"][f] == 2 * ref["ran"][f], (f, ref["ran"], got["ran"])


@pytest.mark.parametrize("pattern", ["filter_only", "all_but_filter", "all"])
def test_filter_on_its_second_stream(gpu_lib, pattern):
    """hyena.FILTER_SIDE_STREAM = True at (B, L, D) = (2, 8192, 128), bf16 autocast: output and every gradient are the one-stream run's bits, under
    three freeze patterns -- the filter's backward runs on the second stream, its consumers and producers on the caller's"""
    import hyena_dna_amd.hyena as H
    from hyena_dna_amd import _castcache
    dev = _dev()
    B, L, D = 2, 8192, 128
    torch.manual_seed(21)
    op = H.HyenaOperator(d_model=D, l_max=L + 2, order=2, filter_order=64, emb_dim=5, short_filter_order=3, modulate=True, w=10).to(dev)
    want = {"filter_only": lambda n: n.startswith("filter_fn."), "all_but_filter": lambda n: not n.startswith("filter_fn."), "all": lambda n: True}[pattern]
    for n, p in op.named_parameters():
        p.requires_grad_(bool(want(n)))
    g = torch.Generator().manual_seed(22)
    u0, dy = torch.randn(B, L, D, generator=g).to(dev), torch.randn(B, L, D, generator=g).to(dev)
    real, streams = H._filter_side_stream, []

    def spy(u, l):
        s = real(u, l)
        streams.append(s)
        return s
    was = H.FILTER_SIDE_STREAM
    res = {}
    try:
        H._filter_side_stream = spy
        for side in (False, True):
            H.FILTER_SIDE_STREAM = side
            del streams[:]
            _castcache.reset()
            op.zero_grad(set_to_none=True)
            u = u0.clone().requires_grad_(pattern != "filter_only")
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = op(u)
            y.float().backward(dy)
            torch.cuda.synchronize()
            assert len(streams) == 1 and (streams[0] is not None) == side
            res[side] = [y.detach(), u.grad] + [p.grad for _, p in op.named_parameters()]
    finally:
        H.FILTER_SIDE_STREAM = was
        H._filter_side_stream = real
    for (n, p), a, b in zip([("y", None), ("u", None)] + list(op.named_parameters()), res[True], res[False]):
        if n == "y" or (n == "u" and pattern != "filter_only") or (p is not None and p.requires_grad):
            assert a is not None and bool(torch.isfinite(a).all()), n
        else:
            assert a is None, n
        assert AL.same_bits(a, b), (n, "the second stream changes the bits")


def test_dropout_seeds_under_graph_replay(gpu_lib):
    """GraphedTrainStep with embed_dropout = resid_dropout = 0.1 (what hg38_hyena.yaml trains with): the seed tensors of the fused dropout are drawn
    INSIDE the captured step -- every backward reads the very tensor its forward drew, every replay draws new values, and the whole sequence
    repeats from torch.manual_seed.  The optimizer's learning rate is 0, so that the parameters stand still and the loss moves with the masks alone."""
    from hyena_dna_amd import _lib
    from hyena_dna_amd.lm import GraphedTrainStep, HyenaDNALM
    dev = _dev()
    B, L, D = 2, 2048, 128
    layer = dict(l_max=L + 2, order=2, filter_order=64, emb_dim=5, short_filter_order=3, modulate=True, w=10)
    ids = torch.randint(7, 11, (B, L), generator=torch.Generator().manual_seed(3)).to(dev)
    names = ("embed_add_norm_fwd", "add_norm_fwd", "embed_add_norm_bwd", "add_norm_bwd")
    real = {n: getattr(_lib, n) for n in names}

    def build_and_replay():
        seen = []

        def spy(n):
            def f(*a, **k):
                if torch.cuda.is_current_stream_capturing():
                    seen.append((n, k.get("dropout_p", 0.0), k.get("seed")))
                return real[n](*a, **k)
            return f
        torch.manual_seed(7)
        m = HyenaDNALM(d_model=D, n_layer=2, d_inner=4 * D, vocab_size=12, layer=layer, resid_dropout=0.1, embed_dropout=0.1,
                       pad_vocab_size_multiple=8).to(dev).train()
        opt = torch.optim.AdamW(m.parameters(), lr=0.0, weight_decay=0.0, capturable=True)
        try:
            for n in names:
                setattr(_lib, n, spy(n))
            step = GraphedTrainStep(m, opt, ids, torch.roll(ids, -1, 1), warmup=2)
        finally:
            for n in names:
                setattr(_lib, n, real[n])
        fwd = [(n, s) for n, p, s in seen if n.endswith("_fwd")]
        bwd = [(n, s) for n, p, s in seen if n.endswith("_bwd")]
        assert all(p == 0.1 and s is not None for _, p, s in seen), seen
        # the first block's norm gathers the embedding; norm2 of block 0, norm1 / norm2 of block 1 and ln_f are add_norm: five seeds
        assert [n for n, _ in fwd] == ["embed_add_norm_fwd"] + ["add_norm_fwd"] * 4 and len(bwd) == 5
        assert len({id(s) for _, s in fwd}) == 5
        for (nf, sf), (nb, sb) in zip(fwd, reversed(bwd)):         # (a)
            assert nb == nf.replace("_fwd", "_bwd") and sb is sf, (nf, nb, "the backward did not get its forward's seed tensor")
        losses, values = [], []
        for _ in range(4):
            losses.append(step().clone())
            torch.cuda.synchronize()
            values.append([int(s.item()) for _, s in fwd])
        step.release()
        return torch.stack(losses).cpu(), values

    losses, values = build_and_replay()
    for j in range(5):                                             # (b)
        col = [v[j] for v in values]
        assert all(a != b for a, b in zip(col, col[1:])), ("seed", j, "is frozen into the graph", col)
    assert len({float(x) for x in losses}) > 1, losses
    assert bool(torch.isfinite(losses).all())
    losses2, values2 = build_and_replay()                          # (c)
    assert torch.equal(losses, losses2) and values == values2, (losses, losses2)
