#!/usr/bin/env python
"""Mint the language-model golden from the REAL reference (imported from /root/reference): ``SimpleLMHeadModel``
(src/models/sequence/simple_lm.py:26-305 -- the reference's own PyTorch restatement of the flash_attn backbone) with the
reference ``HyenaOperator`` as mixer, a hyenadna-tiny-shaped stack (d_model 128, 2 layers, d_inner 512, vocab 12 padded to
16) at L = 4096 (the workspace-free long-convolution plan, whole 16-byte vectors in the shell kernels), fp32 on the CPU:
logits, loss and EVERY parameter gradient.  A second fixture from the same configuration at L = 1023, B = 4 with l_max = L + 3: the shape of the
batches the reference trainer feeds the model (L = max_length - 1, several sequences), where ``HyenaDNALM`` pads to 1024 (lm.HyenaDNALM._aligned_length;
l_max admits 1024, so the route is really taken) and the reference does not.

    python oracle/make_golden_lm.py            # rewrites tests/golden/lm_simple_d128_l4096.pt and lm_simple_d128_l1023_b4*.pt   (build container only)

The second fixture is written in parts of less than 1 MiB each: ``lm_simple_d128_l1023_b4.pt`` holds the configuration, ids, targets, logits, loss and
the names of the part files; ``lm_simple_d128_l1023_b4.partN.pt`` hold the state dict and the gradients, tensor by tensor.  ``tests/lm_golden.py`` puts
them together again.  Only data goes into either fixture.

TEST INFRASTRUCTURE: the fixture pins ``hyena_dna_amd.lm.HyenaDNALM`` on the GPU (tests/test_gpu_contract.py); nothing in the
product imports this file.  Stubs as in oracle/make_golden.py (they touch no arithmetic).
"""
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, import_reference  # noqa: E402

NAME = "lm_simple_d128_l4096.pt"
NAME_ODD = "lm_simple_d128_l1023_b4.pt"              # L = 1023, B = 4, l_max = L + 3, written in parts (PART_BYTES)
PART_BYTES = 900_000                                 # tensor bytes per part file: every file stays under 1 MiB
CFG = dict(d_model=128, n_layer=2, d_inner=512, vocab_size=12, resid_dropout=0.0, embed_dropout=0.0, pad_vocab_size_multiple=8,
           residual_in_fp32=True)
L, B = 4096, 2
LAYER = dict(_name_="hyena", l_max=L + 2, order=2, filter_order=64, emb_dim=5, short_filter_order=3, modulate=True, w=10, lr=6e-4,
             wd=0.0, lr_pos_emb=0.0)


def import_simple_lm():
    import_reference()
    import transformers.tokenization_utils  # noqa: F401  (probes torchvision; must come before the stub below)

    class _SD(torch.nn.Module):                       # torchvision.ops.StochasticDepth with p = 0: identity
        def __init__(self, p, mode):
            super().__init__()

        def forward(self, x):
            return x
    ops = types.ModuleType("torchvision.ops")
    ops.StochasticDepth = _SD
    tv = types.ModuleType("torchvision")
    tv.ops = ops
    sys.modules["torchvision"], sys.modules["torchvision.ops"] = tv, ops
    import src.models.sequence.simple_lm as ref_simple
    return ref_simple


def mint(L, B, l_max):
    """the reference model's results on one (B, L) batch; every fixture starts from the same seeds, so each is independent of what was minted before it"""
    ref_simple = import_simple_lm()
    layer = dict(LAYER, l_max=l_max)
    torch.manual_seed(20240924)
    model = ref_simple.SimpleLMHeadModel(layer=dict(layer), **CFG)
    # the reference initialises every bias to zero (long_conv_lm.py:204-246); give them values so that their gradients and
    # their place in the forward are pinned too
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith(".bias") and "filter_fn.bias" not in n and "norm" not in n and "ln_f" not in n:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    ids = torch.randint(7, 11, (B, L), generator=g)           # A, C, G, T (hg38_char_tokenizer.py:59-66)
    tgt = torch.roll(ids, -1, 1)
    logits = model(ids)[0].logits
    loss = torch.nn.functional.cross_entropy(logits.float().reshape(-1, logits.shape[-1]), tgt.reshape(-1))
    loss.backward()
    out = dict(cfg=CFG, layer={k: v for k, v in layer.items() if k != "_name_"}, L=L, B=B,
               state_dict={k: v.detach().clone() for k, v in model.state_dict().items()},
               ids=ids, targets=tgt, logits=logits.detach().clone(), loss=float(loss),
               grads={n: p.grad.detach().clone() for n, p in model.named_parameters()},
               torch=torch.__version__, note="oracle/make_golden_lm.py: reference SimpleLMHeadModel, fp32, CPU")
    return out, sum(p.numel() for p in model.parameters())


def save_in_parts(out, name):
    """``out`` without its state dict and gradients under ``name``; those, tensor by tensor, in part files of at most PART_BYTES of tensor data"""
    stem = name[:-len(".pt")]
    items = [("state_dict", k, v) for k, v in out["state_dict"].items()] + [("grads", k, v) for k, v in out["grads"].items()]
    parts, size = [dict(state_dict={}, grads={})], 0
    for kind, k, v in items:
        nbytes = v.numel() * v.element_size()
        if size and size + nbytes > PART_BYTES:
            parts.append(dict(state_dict={}, grads={}))
            size = 0
        parts[-1][kind][k] = v
        size += nbytes
    names = [f"{stem}.part{i}.pt" for i in range(len(parts))]
    for stale in os.listdir(OUT):                             # parts of an earlier minting with another split
        if stale.startswith(stem + ".part") and stale not in names:
            os.remove(os.path.join(OUT, stale))
    for n, part in zip(names, parts):
        torch.save(part, os.path.join(OUT, n))
    head = {k: v for k, v in out.items() if k not in ("state_dict", "grads")}
    head["parts"] = names
    torch.save(head, os.path.join(OUT, name))
    return [name] + names


def main():
    out, n_params = mint(L, B, L + 2)
    path = os.path.join(OUT, NAME)
    torch.save(out, path)
    print(NAME, os.path.getsize(path), "loss", out["loss"], "params", n_params)
    out, n_params = mint(1023, 4, 1023 + 3)
    for n in save_in_parts(out, NAME_ODD):
        print(n, os.path.getsize(os.path.join(OUT, n)))
    print(NAME_ODD, "loss", out["loss"], "params", n_params)


if __name__ == "__main__":
    main()
