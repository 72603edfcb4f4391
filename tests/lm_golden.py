"""Shared by the language-model tests: a recorder of the lengths the mixers really run at, and the loader of the goldens minted by oracle/make_golden_lm.py.  A fixture is one file, or -- where one file would be larger than 1 MiB --
a head file that names its part files (``parts``), which hold the state dict and the gradients tensor by tensor."""
import contextlib
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LM_ODD = "lm_simple_d128_l1023_b4.pt"          # reference SimpleLMHeadModel at L = 1023, B = 4, l_max = 1026: HyenaDNALM pads this batch to 1024


def load_lm_golden(name):
    c = torch.load(os.path.join(GOLDEN, name), weights_only=False)
    if "parts" in c:
        c["state_dict"], c["grads"] = {}, {}
        for part in c.pop("parts"):
            p = torch.load(os.path.join(GOLDEN, part), weights_only=False)
            assert not (set(p["state_dict"]) & set(c["state_dict"])) and not (set(p["grads"]) & set(c["grads"])), part
            c["state_dict"].update(p["state_dict"])
            c["grads"].update(p["grads"])
    return c


@contextlib.contextmanager
def mixer_lengths(model):
    """the sequence lengths ``model``'s mixers are really given during a forward (what ``forward`` did, not what ``_aligned_length`` says), one entry per
    mixer call: a pre-hook on the module call, and a wrapper around ``forward_add_norm`` -- the block's fused route calls that method directly and falls
    back to the module call when it answers None, so only an answer is counted there"""
    seen, undo = [], []
    for m in model._mixers():
        h = m.register_forward_pre_hook(lambda mod, args, kwargs: seen.append(args[0].shape[-2]), with_kwargs=True)
        undo.append(h.remove)
        inner = getattr(m, "forward_add_norm", None)
        if inner is not None:
            def wrapped(u, *a, _inner=inner, **kw):
                out = _inner(u, *a, **kw)
                if out is not None:
                    seen.append(u.shape[-2])
                return out
            m.forward_add_norm = wrapped                       # (an instance attribute over the class's method; deleted again below)
            undo.append(lambda m=m: delattr(m, "forward_add_norm"))
    try:
        yield seen
    finally:
        for f in undo:
            f()
