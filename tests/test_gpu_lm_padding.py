"""The two host-side routes between every kernel and every training step of the shipped experiment, on a real MI355X:

* sequence padding (``lm.HyenaDNALM._aligned_length``): the padded run next to the reference's own model at L = 1023, B = 4
  (tests/golden/lm_simple_d128_l1023_b4.pt, oracle/make_golden_lm.py) and next to the unpadded run of the same model on the same batch, at the
  (B, L) the hg38 configurations produce and at the edges of the rule; every case asserts the length it ran at;
* the 16-bit weight shadows (``_castcache``) across hipGraph replays of ``lm.GraphedTrainStep``: an eager evaluation between two replays uses
  exactly the weights a plain cast would give.

Bounds.  fp32 against the reference and padded against unpadded: 2e-5 on the logits, 1e-5 on the loss, 5e-4 per gradient -- what
tests/test_gpu_contract.py::test_lm_vs_reference_simple_lm_golden holds the aligned fixture to (two routes that are each within that of the
reference could be twice as far apart; the one bound is asked for).  bf16 autocast: that test's 16-bit bounds, 5e-2 / 2e-2 / 0.1.  The cache
and the bidirectional model: bit for bit.

Measured on an MI355X when these tests were written (every test prints its figures; run with -s).  fp32 against the reference: logits 3.3e-7,
loss 8.8e-8, worst gradient 9.6e-7, padded and unpadded alike; bf16: 3.4e-3 / 4.8e-5 / 1.5e-2.  Padded against unpadded, fp32: logits
1.5e-7 ... 5.5e-7 (the largest at (8, 32767) d 256; 3.7e-7 at (2, 159999)), loss equal or one ulp apart, worst gradient 1.1e-6 ((4, 8191) and
(1, 32767)); bf16: logits <= 1.7e-3, worst gradient 3.3e-4.  The whole file: ~ 9 s.

Small model throughout (d_model 128, 2 layers, d_inner 512), dropout off."""
import pytest
import torch

import hyena_dna_amd.lm as LM
from hyena_dna_amd import _castcache as CC
from tests.lm_golden import LM_ODD, load_lm_golden, mixer_lengths

pytestmark = pytest.mark.gpu

TOL32 = dict(logits=2e-5, loss=1e-5, grad=5e-4)
TOL16 = dict(logits=5e-2, loss=2e-2, grad=0.1)


def _dev():
    return torch.device("cuda", 0)


def _rel(a, b):
    a, b = a.detach().to(_dev(), torch.float64), b.detach().to(_dev(), torch.float64)
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _model(l_max, d=128, n_layer=2, order=2, seed=0, **layer_kw):
    torch.manual_seed(seed)
    layer = dict(l_max=l_max, order=order, filter_order=64, emb_dim=5, short_filter_order=3, modulate=True, w=10, lr=6e-4, wd=0.0, lr_pos_emb=0.0,
                 **layer_kw)
    model = LM.HyenaDNALM(d_model=d, n_layer=n_layer, d_inner=4 * d, vocab_size=12, layer=layer, resid_dropout=0.0, embed_dropout=0.0,
                          pad_vocab_size_multiple=8, fused_dropout_add_ln=True, residual_in_fp32=True)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():            # the LM initialises every bias to zero: give them values, so that their place in the padded run is checked too
        for n, p in model.named_parameters():
            if n.endswith(".bias") and "filter_fn.bias" not in n and "norm" not in n and "ln_f" not in n:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    return model


def _batch(B, L, seed):
    ids = torch.randint(7, 11, (B, L), generator=torch.Generator().manual_seed(seed)).to(_dev())
    return ids, torch.roll(ids, -1, 1)


def _run(model, ids, tgt, bf16=False):
    """one forward + backward: (logits fp32, loss, {name: grad}, the sequence lengths the mixers were given)"""
    model.zero_grad(set_to_none=True)
    with mixer_lengths(model) as seen, torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        logits = model(ids)[0].logits
    loss = torch.nn.functional.cross_entropy(logits.float().reshape(-1, logits.shape[-1]), tgt.reshape(-1))
    loss.backward()
    grads = {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None}
    return logits.detach().float().clone(), loss.item(), grads, seen


def _check(tag, got, ref, tol):
    """every figure printed, then all of them asserted at once (one run shows everything a case has to say)"""
    (la, lossa, ga), (lb, lossb, gb) = got, ref
    assert la.shape == lb.shape and set(ga) == set(gb), (tag, set(ga) ^ set(gb))
    assert bool(torch.isfinite(la).all())
    figs = {"logits": (_rel(la, lb), tol["logits"]), "loss": (abs(lossa - lossb) / abs(lossb), tol["loss"])}
    for n in gb:
        figs["grad " + n] = (_rel(ga[n], gb[n]), tol["grad"])
    worst = max((v for k, (v, _) in figs.items() if k.startswith("grad ")), default=0.0)
    print(f"[{tag}] logits {figs['logits'][0]:.3e} loss {figs['loss'][0]:.3e} ({lossa!r} vs {lossb!r}) worst grad {worst:.3e}", flush=True)
    bad = {k: v for k, (v, bound) in figs.items() if not v < bound}
    assert not bad, (tag, bad)


@pytest.fixture()
def rule(monkeypatch):
    """the single-sequence rule at its shipped values, whatever the environment of the run says"""
    monkeypatch.setattr(LM, "_PAD_SINGLE_MIN", 8192)
    monkeypatch.setattr(LM, "_PAD_SINGLE_ROWS", 4096)
    return monkeypatch


def test_odd_length_batch_vs_reference_simple_lm_golden(gpu_lib, rule):
    """HyenaDNALM on the reference's 4 x 1023 batch against SimpleLMHeadModel's logits, loss and every gradient (fp32, CPU): add + LayerNorm fused
    and unfused, padded to 1024 and as it comes; then bf16 autocast, padded, at the 16-bit bounds."""
    dev = _dev()
    c = load_lm_golden(LM_ODD)
    ids, tgt = c["ids"].to(dev), c["targets"].to(dev)
    assert ids.shape == (4, 1023) and c["layer"]["l_max"] == 1026
    ref = (c["logits"], c["loss"], c["grads"])
    for fused_ln in (True, False):
        model = LM.HyenaDNALM(layer=dict(c["layer"]), fused_dropout_add_ln=fused_ln, **c["cfg"])
        model.load_state_dict(c["state_dict"], strict=True)
        model = model.to(dev)
        for pad in (True, False):
            rule.setattr(LM, "PAD_SEQUENCES", pad)
            lp = 1024 if pad else 1023
            assert model._aligned_length(ids) == lp
            logits, loss, grads, seen = _run(model, ids, tgt)
            assert seen == [lp, lp] and logits.shape == (4, 1023, 16)
            assert set(grads) == set(c["grads"])
            _check(f"reference fp32 fused_ln={fused_ln} pad={pad}", (logits, loss, grads), ref, TOL32)
    rule.setattr(LM, "PAD_SEQUENCES", True)
    logits, loss, grads, seen = _run(model, ids, tgt, bf16=True)
    assert seen == [1024, 1024]
    _check("reference bf16 pad=True", (logits, loss, grads), ref, TOL16)


# (B, L, d_model, order, the length the padded run must take)
CASES = [(8, 1023, 128, 2, 1024),            # hg38 batches: max_length 1024 / 8192 / 32768, L = max_length - 1
         (4, 8191, 128, 2, 8192),
         (8, 32767, 256, 2, 32768),          # hyenadna-small-32k; the workspace-free plan at its largest size
         (2, 159999, 128, 2, 160000),        # two-level plan, mixed-radix columns
         (2, 65, 128, 2, 128),               # one tile + 1: the shortest padded length
         (3, 127, 128, 2, 128),
         (2, 32831, 128, 2, 32832),          # the first padded length of the two-level plan
         (1, 12287, 128, 2, 12288),          # one long sequence: padded where the padded length is a multiple of 4096 ...
         (1, 32767, 128, 2, 32768),
         (1, 8191, 128, 2, 8191),            # ... and only from 8192 positions on
         (4, 1023, 128, 3, 1024)]            # order 3: the channel-major order-N route


def _padded_vs_unpadded(rule, B, L, d, order, Lp, bf16):
    model = _model(Lp + 2, d=d, order=order, seed=L % 1000).to(_dev())
    ids, tgt = _batch(B, L, seed=L + B)
    res = {}
    for pad in (False, True):
        rule.setattr(LM, "PAD_SEQUENCES", pad)
        want = Lp if pad else L
        assert model._aligned_length(ids) == want
        logits, loss, grads, seen = _run(model, ids, tgt, bf16=bf16)
        assert seen == [want, want] and logits.shape == (B, L, 16)
        res[pad] = (logits, loss, grads)
    _check(f"padded vs unpadded ({B}, {L}) d={d} order={order} {'bf16' if bf16 else 'fp32'}", res[True], res[False], TOL16 if bf16 else TOL32)
    del model, res
    torch.cuda.empty_cache()


@pytest.mark.parametrize("B,L,d,order,Lp", CASES)
def test_padded_vs_unpadded_fp32(gpu_lib, rule, B, L, d, order, Lp):
    """same model, same batch, padding on and off: logits, loss, every parameter gradient and the set of parameters that got one"""
    _padded_vs_unpadded(rule, B, L, d, order, Lp, bf16=False)


@pytest.mark.parametrize("B,L,d,order,Lp", [CASES[0], CASES[2], CASES[3]])
def test_padded_vs_unpadded_bf16_autocast(gpu_lib, rule, B, L, d, order, Lp):
    _padded_vs_unpadded(rule, B, L, d, order, Lp, bf16=True)


def test_a_single_sequence_of_999999_stays_as_it_is(gpu_lib, rule):
    """1 000 000 is not a multiple of 4096: the padded count would still need the two-level weight-gradient plan (rule only, nothing runs)"""
    rule.setattr(LM, "PAD_SEQUENCES", True)
    model = _model(1000002, n_layer=1)
    assert model._aligned_length(torch.zeros(1, 999999, dtype=torch.long, device=_dev())) == 999999
    assert model._aligned_length(torch.zeros(2, 999999, dtype=torch.long, device=_dev())) == 1000000


def test_bidirectional_stack_is_not_padded_on_the_gpu(gpu_lib, rule):
    """layer.bidirectional=True: the model runs at the caller's length, padding on and off are the same route -- the same bits"""
    B, L = 3, 1023
    model = _model(L + 3, bidirectional=True).to(_dev())
    ids, _ = _batch(B, L, seed=11)
    out = {}
    for pad in (True, False):
        rule.setattr(LM, "PAD_SEQUENCES", pad)
        assert model._aligned_length(ids) == L
        with mixer_lengths(model) as seen, torch.no_grad():
            out[pad] = model(ids)[0].logits.clone()
        assert seen == [L, L]
    assert out[True].shape == (B, L, 16) and bool(torch.isfinite(out[True]).all()) and torch.equal(out[True], out[False])


def test_training_with_and_without_padding(gpu_lib, rule):
    """6 eager AdamW steps under bf16 autocast on 4 x 1023 batches from the same seed, padding on and off: the losses step by step, at the
    16-bit bound on a loss (2e-2)"""
    B, L, steps = 4, 1023, 6
    batches = [_batch(B, L, seed=100 + i) for i in range(steps)]
    losses = {}
    for pad in (True, False):
        rule.setattr(LM, "PAD_SEQUENCES", pad)
        model = _model(L + 3, seed=3).to(_dev())
        opt = torch.optim.AdamW(model.parameters(), lr=6e-4, weight_decay=0.1)
        assert model._aligned_length(batches[0][0]) == (1024 if pad else L)
        losses[pad] = []
        for ids, tgt in batches:
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = model.loss(ids, tgt)
            loss.backward()
            opt.step()
            losses[pad].append(loss.item())
    print("[training] padded", losses[True], "unpadded", losses[False], flush=True)
    assert all(a == a and abs(a - b) < 2e-2 * abs(b) for a, b in zip(losses[True], losses[False])), losses
    assert losses[False][-1] < losses[False][0]                              # (they are training steps: the loss moves)


def test_cast_cache_across_graph_replays(gpu_lib, monkeypatch):
    """A replay of lm.GraphedTrainStep updates the parameters on the device and moves neither their version counters nor their addresses.  An eager
    evaluation between two replays must still use exactly ``p.to(bf16)`` of the CURRENT weights: its loss equals, bit for bit, the loss of the same
    call with the cache switched off -- after every replay and after release().  The refresh is part of the captured step (two replays back to back:
    the shadows hold the weights the second one started from), and each eager evaluation after a replay costs one batched refresh, not one per use."""
    from hyena_dna_amd.lm import GraphedTrainStep
    monkeypatch.setattr(CC, "ENABLED", True)
    dev = _dev()
    B, L = 2, 2048
    model = _model(L + 2, seed=7).to(dev)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.1, capturable=True)
    batches = [_batch(B, L, seed=200 + i) for i in range(6)]
    ev_ids, ev_tgt = _batch(B, L, seed=300)

    def evaluate(cache):
        monkeypatch.setattr(CC, "ENABLED", cache)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return model.loss(ev_ids, ev_tgt).clone()

    def check(tag):
        n0 = CC.stats()["bulk_refreshes"]
        cached = evaluate(True)
        n1 = CC.stats()["bulk_refreshes"]
        again = evaluate(True)                                               # (a second evaluation without a replay in between: all hits)
        assert CC.stats()["bulk_refreshes"] == n1
        plain = evaluate(False)
        monkeypatch.setattr(CC, "ENABLED", True)
        print(f"[cast cache] {tag}: cached {cached.item()!r} plain {plain.item()!r} refreshes {n1 - n0}", flush=True)
        assert bool(torch.isfinite(plain)) and torch.equal(cached, plain) and torch.equal(again, plain), (tag, cached.item(), plain.item())
        assert n1 - n0 == 1, (tag, n1 - n0)
        return plain.item()

    evaluate(True)                                                           # registers every shadow (first uses: one by one)
    step = GraphedTrainStep(model, opt, *batches[0], warmup=2)
    seen = []
    for i, (ids, tgt) in enumerate(batches[:4]):
        step(ids, tgt)
        seen.append(check(f"after replay {i}"))
    assert len(set(seen)) == 4                                               # (the replays do train: the evaluation loss moves every time)
    # two replays back to back: the second one's captured refresh put the weights it started from into the shadows, on the device
    w = model.backbone.layers[0].mlp.fc1.weight
    step(*batches[4])
    torch.cuda.synchronize(dev)
    before = w.detach().clone()
    step(*batches[5])
    torch.cuda.synchronize(dev)
    shadow = CC._entries[(id(w), torch.bfloat16)].shadow
    assert torch.equal(shadow, before.to(torch.bfloat16)) and not torch.equal(shadow, w.detach().to(torch.bfloat16))
    check("after two replays back to back")
    step(*batches[0])
    step.release()
    check("after release")
