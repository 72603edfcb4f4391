#!/usr/bin/env python
"""Mint the optimizer parameter groups of the REAL reference (train.py:443-468, the group-building lines of
`SequenceLightningModule.configure_optimizers`) on the reference's own model -- SimpleLMHeadModel with the reference
HyenaOperator and its `_optim` tags -- for the hg38 experiment config with `model.d_model=64 optimizer.lr=3e-4`, and store
them as tests/golden/hg38_optimizer_groups.json: per group its hyperparameters and the names of its parameters, in order.

    python oracle/make_golden_optimizer_groups.py          (build container only: needs the reference checkout)

tests/test_runner.py checks runner.build_optimizer on HyenaDNALM against this file."""
import importlib
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("HYENA_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "hg38_optimizer_groups.json")
OVERRIDES = ["model.d_model=64", "optimizer.lr=3e-4"]


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _get(path):
    mod, _, attr = path.rpartition(".")
    return getattr(importlib.import_module(mod), attr)


def main():
    sys.path[:0] = [ROOT, REF]
    import torch
    # what the reference's model modules import but do not need for building a model
    _stub("hydra", utils=_stub("hydra.utils", get_method=_get, get_class=_get))
    _stub("omegaconf", ListConfig=list, DictConfig=type("DictConfig", (dict,), {}), OmegaConf=object)
    _stub("pytorch_lightning", utilities=_stub("pytorch_lightning.utilities", rank_zero_only=lambda f: f))
    _stub("opt_einsum", contract=torch.einsum)
    import transformers.tokenization_utils  # noqa: F401

    class _SD(torch.nn.Module):
        def __init__(self, p, mode):
            super().__init__()

        def forward(self, x):
            return x

    _stub("torchvision", ops=_stub("torchvision.ops", StochasticDepth=_SD))
    import src.models.sequence.simple_lm as ref_simple
    from hyena_dna_amd import runner
    cfg = runner.compose(os.path.join(REF, "configs"), overrides=OVERRIDES)
    m = dict(cfg["model"])
    m.pop("_name_")
    layer = dict(m.pop("layer"))
    for k in ("fused_mlp", "fused_dropout_add_ln", "checkpoint_mixer", "checkpoint_mlp"):
        m.pop(k)
    ref_model = ref_simple.SimpleLMHeadModel(layer=layer, **m)
    # --- train.py:443-468, the reference's lines on the reference's model (hparams.optimizer = cfg["optimizer"]) ---
    hp_opt = dict(cfg["optimizer"])
    hp_opt.pop("_name_")
    all_params = list(ref_model.named_parameters())
    groups = [({k: v for k, v in hp_opt.items()}, [n for n, p in all_params if not hasattr(p, "_optim")])]
    hps = [getattr(p, "_optim") for _, p in all_params if hasattr(p, "_optim")]
    hps = [dict(s) for s in sorted(list(dict.fromkeys(frozenset(hp.items()) for hp in hps)))]
    for hp in hps:
        groups.append(({**hp_opt, **hp}, [n for n, p in all_params if getattr(p, "_optim", None) == hp]))
    doc = {"experiment": "hg38/hg38_hyena", "overrides": OVERRIDES,
           "source": "the reference's configure_optimizers group lines (train.py:443-468) on its SimpleLMHeadModel "
                     "(oracle/make_golden_optimizer_groups.py)",
           "groups": [{"hparams": hp, "params": names} for hp, names in groups]}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(OUT, os.path.getsize(OUT), [len(n) for _, n in groups])


if __name__ == "__main__":
    main()
