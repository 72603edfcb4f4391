"""The autograd layer (the 17 torch.autograd.Functions of hyena_dna_amd) on the CPU-emulated kernels: registry, freeze-pattern sweep, no_grad
forward, gradient layouts and retained graphs of tests/autograd_local.py.  tests/test_gpu_autograd_local.py runs the same suites on the gfx950
library.  Tables, counts and run times: profiles/autograd_local.md."""
import os

import pytest
import torch

from tests import autograd_local as AL

DEV = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CASES = [(key, i) for key, e in AL.REGISTRY.items() for i in range(len(e.cases(False)))]
_case_ids = [f"{k}-c{i}" for k, i in _CASES]


def test_registry_lists_every_function():
    """a scan of the torch.autograd.Function subclasses under hyena_dna_amd/ against the registry: a new Function needs an entry"""
    found = AL.function_classes()
    assert len(found) == 17, sorted(found)
    assert {e.func for e in AL.REGISTRY.values()} == set(found)
    for key, e in AL.REGISTRY.items():
        assert e.cases(False) and e.cases(True) and e.patterns(), key
        assert e.act is None or e.act in e.inputs
        for members in e.groups.values():
            assert set(members) <= set(e.inputs), key


def test_oracle_tolerances_are_the_contract_files():
    src = open(os.path.join(ROOT, "tests", "test_gpu_contract.py")).read()
    for key, (line, value) in AL.CONTRACT_SOURCE.items():
        assert line in src, (key, line)
        assert float(line.replace("(", " ").replace(",", " ").split()[-1 if key != "core_16" else 3]) == value, (key, line, value)


def test_patterns_cover_what_the_sweep_promises():
    small = AL.patterns(("a", "b", "c"), {}, "a")
    assert len(small) == 7
    ins = tuple("abcdef")
    big = dict(AL.patterns(ins, {"grp": ("b", "c")}, "a"))
    for n in ins:
        assert frozenset({n}) in big.values() and frozenset(set(ins) - {n}) in big.values()
    assert frozenset(ins) in big.values() and frozenset("bc") in big.values() and frozenset("abc") in big.values()
    assert all(big.values()) and len(set(big.values())) == len(big)


@pytest.mark.parametrize("key,i,name", [p[:3] for p in AL.sweep_params(False)], ids=[p[3] for p in AL.sweep_params(False)])
def test_freeze_pattern(emu_backend, key, i, name):
    AL.suite_pattern(emu_backend, DEV, key, i, name)


@pytest.mark.parametrize("key,i", _CASES, ids=_case_ids)
def test_forward_under_no_grad(emu_backend, key, i):
    AL.suite_no_grad(emu_backend, DEV, key, i)


@pytest.mark.parametrize("key,i", _CASES, ids=_case_ids)
def test_gradient_layouts(emu_backend, key, i):
    AL.suite_layouts(emu_backend, DEV, key, i)


_MIXER_CASES = [(k, i) for k, i in _CASES if k in AL.MIXERS]


@pytest.mark.parametrize("key,i", _MIXER_CASES, ids=[f"{k}-c{i}" for k, i in _MIXER_CASES])
def test_retained_graph(emu_backend, monkeypatch, key, i):
    """three backward passes over one graph; B >= 2 on the on-chip plan keeps the filter spectrum for the first one alone [spectra=absent]"""
    AL.suite_retained(emu_backend, DEV, key, i, mp=monkeypatch)


@pytest.mark.parametrize("saved", [True, False], ids=["saved[spectra=absent]", "recompute"])
@pytest.mark.parametrize("key", list(AL.TWO_LEVEL))
def test_retained_graph_two_level(emu_backend, monkeypatch, key, saved):
    how = AL.suite_retained_two_level(emu_backend, DEV, monkeypatch, key, saved)
    assert how.startswith("spectra=absent") == saved


_LM = [(cfg, ck) for cfg in AL.LM_GRID for ck in AL.CKPT]


@pytest.mark.parametrize("cfg,ck", _LM, ids=[AL.lm_id(*c) + f"-mixer{int(k[0])}-mlp{int(k[1])}" for c, k in _LM])
def test_lm_checkpointing(emu_backend, cfg, ck):
    AL.suite_lm_checkpoint(emu_backend, DEV, cfg, ck)


_LMF = [(cfg, ck, f) for cfg in AL.LM_CROSS for ck in AL.CKPT for f in ("biases_only", "filter_only")]


@pytest.mark.parametrize("cfg,ck,freeze", _LMF, ids=[AL.lm_id(*c) + f"-mixer{int(k[0])}-mlp{int(k[1])}-{f}" for c, k, f in _LMF])
def test_lm_checkpointing_under_freezing(emu_backend, cfg, ck, freeze):
    AL.suite_lm_checkpoint(emu_backend, DEV, cfg, ck, freeze)


_LMG = [(cfg, ck, f) for cfg in AL.LM_CROSS for ck in [(False, False), (True, True)] for f in ("out_proj_bias_only", "fc2_bias_only")]


@pytest.mark.parametrize("cfg,ck,freeze", _LMG, ids=[AL.lm_id(*c) + f"-mixer{int(k[0])}-mlp{int(k[1])}-{f}" for c, k, f in _LMG])
def test_lm_bias_only_with_and_without_the_side_table(emu_backend, cfg, ck, freeze):
    AL.suite_lm_gradsum(emu_backend, DEV, cfg, ck, freeze)


def test_every_dropout_call_draws_a_seed_of_its_own(emu_backend, monkeypatch):
    """two calls of the fused dropout + add + LayerNorm after one torch.manual_seed: two seed tensors with two values (a seed drawn once, at import
    or at the first call, would repeat the mask in every layer and every step), each handed to its own backward, and the pair repeats from the seed"""
    from hyena_dna_amd.block import dropout_add_layer_norm
    seen = []
    for name in ("add_norm_fwd", "add_norm_bwd"):
        real = getattr(emu_backend, name)
        monkeypatch.setattr(emu_backend, name, lambda *a, _n=name, _r=real, **k: (seen.append((_n, k.get("seed"))), _r(*a, **k))[1])
    x = torch.randn(3, 23, 64, requires_grad=True)
    w, b = torch.ones(64, requires_grad=True), torch.zeros(64, requires_grad=True)
    values = []
    for _ in range(2):
        del seen[:]
        torch.manual_seed(5)
        y1 = dropout_add_layer_norm(x, None, w, b, 0.1, 1e-5, prenorm=False, residual_in_fp32=True)
        y2 = dropout_add_layer_norm(y1, None, w, b, 0.1, 1e-5, prenorm=False, residual_in_fp32=True)
        y2.sum().backward()
        (f1, s1), (f2, s2), (b2, t2), (b1, t1) = seen
        assert (f1, f2, b2, b1) == ("add_norm_fwd", "add_norm_fwd", "add_norm_bwd", "add_norm_bwd")
        assert s1 is not s2 and int(s1) != int(s2) and t1 is s1 and t2 is s2
        values.append((int(s1), int(s2)))
    assert values[0] == values[1]
