"""HyenaDNALM pads batches of several odd-length sequences to a multiple of 64 positions (round 6, lm.HyenaDNALM._aligned_length): the reference
trainer's batches are (B, max_length - 1) (hg38_dataset.py:222, hg38_hyena.yaml:47-48).  Every operation of the model is causal or per-position,
so the padded run must give the unpadded run's logits, loss and gradients -- checked here under the CPU emulation of the kernels; against the
reference's own model at L = 1023, B = 4 (tests/golden/lm_simple_d128_l1023_b4.pt, oracle/make_golden_lm.py), padded and unpadded; a stack that
is not causal (bidirectional filter) is not padded; and the routes that must not pad really run the mixers at the caller's length."""
import pytest
import torch

import hyena_dna_amd.lm as LM
from tests.lm_golden import LM_ODD, load_lm_golden, mixer_lengths


def _model(L, d=64, n_layer=2, seed=0, l_max=None, max_position_embeddings=0, **layer_kw):
    torch.manual_seed(seed)
    layer = dict(l_max=L + 3 if l_max is None else l_max, order=2, filter_order=64, emb_dim=5, short_filter_order=3, modulate=True, w=10, lr=6e-4,
                 wd=0.0, lr_pos_emb=0.0, **layer_kw)
    return LM.HyenaDNALM(d_model=d, n_layer=n_layer, d_inner=4 * d, vocab_size=12, layer=layer, resid_dropout=0.0, embed_dropout=0.0,
                         pad_vocab_size_multiple=8, fused_dropout_add_ln=True, residual_in_fp32=True,
                         max_position_embeddings=max_position_embeddings)


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("B,L", [(3, 127), (2, 191), (1, 189)])
def test_padded_batch_equals_unpadded_batch(emu_backend, monkeypatch, B, L):
    model = _model(L)
    g = torch.Generator().manual_seed(L)
    ids = torch.randint(7, 11, (B, L), generator=g)
    tgt = torch.roll(ids, -1, 1)
    res = {}
    monkeypatch.setattr(LM, "_PAD_SINGLE_MIN", 100)             # (B = 1: a single sequence counts as long from here on)
    monkeypatch.setattr(LM, "_PAD_SINGLE_ROWS", 64)
    for pad in (True, False):
        monkeypatch.setattr(LM, "PAD_SEQUENCES", pad)
        assert model._aligned_length(ids) == (L + (-L) % 64 if pad else L)
        model.zero_grad(set_to_none=True)
        logits = model(ids)[0].logits
        assert logits.shape == (B, L, 16)
        loss = LM.token_cross_entropy(logits, tgt)
        loss.backward()
        res[pad] = (logits.detach().clone(), loss.item(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    (la, lossa, ga), (lb, lossb, gb) = res[True], res[False]
    assert ((la - lb).norm() / lb.norm()).item() < 2e-5 and abs(lossa - lossb) < 1e-5 * abs(lossb)
    assert set(ga) == set(gb)
    for n in gb:
        e = ((ga[n] - gb[n]).norm() / gb[n].norm().clamp_min(1e-20)).item()
        assert e < 2e-4, (n, e)


def test_padding_only_where_it_applies(emu_backend, monkeypatch):
    monkeypatch.setattr(LM, "PAD_SEQUENCES", True)
    model = _model(127)                                                   # l_max = 130 admits 128
    assert model._aligned_length(torch.zeros(2, 127, dtype=torch.long)) == 128
    assert model._aligned_length(torch.zeros(1, 127, dtype=torch.long)) == 127        # one short sequence: its rows are aligned anyway
    monkeypatch.setattr(LM, "_PAD_SINGLE_MIN", 100)                                   # (one LONG sequence is padded: the odd weight-gradient products ...
    monkeypatch.setattr(LM, "_PAD_SINGLE_ROWS", 128)                                  #  ... where the padded length is a multiple of the slice grid)
    assert model._aligned_length(torch.zeros(1, 127, dtype=torch.long)) == 128
    monkeypatch.setattr(LM, "_PAD_SINGLE_ROWS", 4096)
    assert model._aligned_length(torch.zeros(1, 127, dtype=torch.long)) == 127
    monkeypatch.setattr(LM, "_PAD_SINGLE_MIN", 8192)
    big = _model(32767, d=64, n_layer=1)
    assert big._aligned_length(torch.zeros(1, 32767, dtype=torch.long)) == 32768 and big._aligned_length(torch.zeros(1, 32700, dtype=torch.long)) == 32700
    assert model._aligned_length(torch.zeros(4, 128, dtype=torch.long)) == 128
    assert model._aligned_length(torch.zeros(4, 33, dtype=torch.long)) == 33          # shorter than one 64-position tile
    tight = _model(124)                                                   # l_max = 127 < 128: the operator would truncate -> not padded
    assert tight._aligned_length(torch.zeros(2, 125, dtype=torch.long)) == 125


@pytest.mark.parametrize("pad", [True, False])
def test_odd_length_batch_matches_reference_simple_lm_golden(emu_backend, monkeypatch, pad):
    """HyenaDNALM on the reference's batch of 4 x 1023 (l_max 1026 admits 1024), padded to 1024 and as it comes: logits, loss and every gradient
    against the reference's own model, at the bounds tests/test_lm_golden_emu.py holds the aligned fixture to.  (The reference never pads: the
    padded route is compared with a run that has no pad positions at all, so what they leak into a gradient is bounded here.)"""
    monkeypatch.setattr(LM, "PAD_SEQUENCES", pad)
    c = load_lm_golden(LM_ODD)
    assert c["ids"].shape == (4, 1023) and c["layer"]["l_max"] == 1026
    model = LM.HyenaDNALM(layer=dict(c["layer"]), fused_dropout_add_ln=True, **c["cfg"])
    model.load_state_dict(c["state_dict"], strict=True)
    assert model._aligned_length(c["ids"]) == (1024 if pad else 1023)
    with mixer_lengths(model) as seen:
        logits = model(c["ids"])[0].logits
    assert seen == [1024 if pad else 1023] * 2 and logits.shape == (4, 1023, 16)
    loss = torch.nn.functional.cross_entropy(logits.float().reshape(-1, logits.shape[-1]), c["targets"].reshape(-1))
    loss.backward()
    print("pad", pad, "logits", _rel(logits, c["logits"]), "loss", loss.item(), c["loss"])
    assert _rel(logits, c["logits"]) < 5e-6
    assert abs(loss.item() - c["loss"]) < 1e-6 * abs(c["loss"]) + 1e-7
    grads = {n: p.grad for n, p in model.named_parameters()}
    assert set(grads) == set(c["grads"])
    for n, g in c["grads"].items():
        e = _rel(grads[n], g)
        print("pad", pad, n, e)
        assert e < 2e-5, (n, e)


@pytest.mark.parametrize("B,L", [(3, 127), (2, 191)])
def test_bidirectional_stack_is_not_padded(emu_backend, monkeypatch, B, L):
    """layer.bidirectional=True centres the input in a 2 L window (HyenaFilter.forward): the padded length would move every output, so such a
    model runs at the caller's length whatever PAD_SEQUENCES says -- the two settings are the same route, bit for bit."""
    model = _model(L, bidirectional=True)
    assert all(m.filter_fn.bidirectional for m in model._mixers())
    ids = torch.randint(7, 11, (B, L), generator=torch.Generator().manual_seed(L))
    out = {}
    for pad in (True, False):
        monkeypatch.setattr(LM, "PAD_SEQUENCES", pad)
        assert model._aligned_length(ids) == L
        with mixer_lengths(model) as seen, torch.no_grad():
            out[pad] = model(ids)[0].logits.clone()
        assert seen == [L, L]
    assert out[True].shape == (B, L, 16) and torch.equal(out[True], out[False])
    # (a mixer that is not a HyenaOperator is not known to be causal: not padded either)
    monkeypatch.setattr(LM, "PAD_SEQUENCES", True)
    causal = _model(L)
    assert causal._aligned_length(ids) == L + (-L) % 64
    causal.backbone.layers[1].mixer = torch.nn.Identity()
    assert causal._aligned_length(ids) == L


@pytest.mark.parametrize("B,L", [(3, 127), (2, 191)])
def test_padded_logits_do_not_depend_on_the_pad_tokens(emu_backend, monkeypatch, B, L):
    """The padded route's logits at positions < L against a run, padding off, on the same ids extended by hand to the padded length with RANDOM
    tokens (the route pads with a constant) and cut back to L: nothing that follows position L reaches a position before it.  Bounds of
    test_padded_batch_equals_unpadded_batch."""
    model = _model(L)
    g = torch.Generator().manual_seed(1000 + L)
    ids = torch.randint(7, 11, (B, L), generator=g)
    Lp = L + (-L) % 64
    tail = torch.randint(1, 12, (B, Lp - L), generator=g)
    assert bool((tail != 0).any())
    monkeypatch.setattr(LM, "PAD_SEQUENCES", True)
    assert model._aligned_length(ids) == Lp
    with torch.no_grad():
        padded = model(ids)[0].logits
        monkeypatch.setattr(LM, "PAD_SEQUENCES", False)
        by_hand = model(torch.cat([ids, tail], 1))[0].logits
    assert padded.shape == (B, L, 16) and by_hand.shape == (B, Lp, 16)
    e = _rel(padded, by_hand[:, :L])
    print("padded vs hand-extended", (B, L), e)
    assert e < 2e-5
    # per position, so that a leak into the last few positions cannot hide in the norm over all of them
    num = (padded.double() - by_hand[:, :L].double()).norm(dim=-1)
    den = by_hand[:, :L].double().norm(dim=-1).clamp_min(1e-30)
    assert (num / den).max().item() < 2e-5


def test_routes_that_must_not_pad_run_the_mixers_at_the_callers_length(emu_backend, monkeypatch):
    """explicit position_ids, a prefill with inference_params, an l_max or a position-embedding table that does not admit the padded length:
    `forward` gives the mixers the L it was given (and the plain call of the same model the padded one, so the hook is known to see padding)"""
    from hyena_dna_amd.inference import InferenceParams
    monkeypatch.setattr(LM, "PAD_SEQUENCES", True)
    B, L = 2, 127
    ids = torch.randint(7, 11, (B, L), generator=torch.Generator().manual_seed(5))

    def lengths(model, **kw):
        with mixer_lengths(model) as seen, torch.no_grad():
            logits = model(ids, **kw)[0].logits
        assert logits.shape == (B, L, 16)
        return seen

    model = _model(L)
    assert model._aligned_length(ids) == 128 and lengths(model) == [128, 128]
    assert lengths(model, position_ids=torch.arange(L).expand(B, L)) == [L, L]
    ip = InferenceParams(max_seqlen=128, max_batch_size=B)
    ip.key_value_memory_dict = model.allocate_inference_cache(B, 128)
    assert lengths(model, inference_params=ip) == [L, L]
    tight = _model(L, l_max=L)                                             # l_max = 127 < 128
    assert tight._aligned_length(ids) == L and lengths(tight) == [L, L]
    wide_pos = _model(L, max_position_embeddings=128)                      # the table admits 128: padded
    assert wide_pos._aligned_length(ids) == 128 and lengths(wide_pos) == [128, 128]
    short_pos = _model(L, max_position_embeddings=L)                       # the table ends at 127: not padded
    assert short_pos._aligned_length(ids) == L and lengths(short_pos) == [L, L]
