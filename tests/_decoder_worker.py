"""Worker of tests/test_pool_emu.py: hyena_dna_amd.classifier.SequenceDecoder against the UNMODIFIED reference class
src.tasks.decoders.SequenceDecoder (from the reference checkout), fp32 on CPU tensors.  Build container only."""
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("HYENA_REFERENCE", "/root/reference")


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


CASES = [
    # mode, constructor l_output, use_lengths, call keywords
    ("last", 0, False, {}), ("last", 1, False, {}), ("last", 3, False, {}), ("last", None, False, {}), ("last", None, False, {"l_output": 2}),
    ("first", 0, False, {}), ("first", 2, False, {}), ("first", None, False, {"l_output": 4}),
    ("pool", 0, False, {}), ("pool", 1, False, {}), ("pool", None, False, {"l_output": 1}),
    ("sum", 0, False, {}), ("sum", 1, False, {}),
    ("last", 0, True, {"lengths": [3, 9, 5]}), ("last", 2, True, {"lengths": [3, 9, 5]}), ("first", 2, True, {"lengths": [3, 9, 5]}),
    ("pool", 0, True, {"lengths": [3, 9, 1]}), ("sum", 1, True, {"lengths": [3, 9, 1]}),
    ("last", 0, False, {"lengths": [3, 9, 5]}),          # lengths without use_lengths: ignored, as in the reference
    ("pool", 0, False, {"mask": "prefix"}), ("pool", 1, False, {"mask": "prefix"}), ("pool", None, False, {"mask": "prefix"}),
]


def main():
    sys.path[:0] = [ROOT, REF]
    # inert stand-ins for packages that are not installed here; they touch no arithmetic
    _stub("hydra", utils=_stub("hydra.utils", get_method=None, get_class=None))
    _stub("omegaconf", ListConfig=list, DictConfig=type("DictConfig", (dict,), {}), OmegaConf=object)
    _stub("pytorch_lightning", utilities=_stub("pytorch_lightning.utilities", rank_zero_only=lambda f: f))
    _stub("opt_einsum", contract=torch.einsum)
    from src.tasks.decoders import SequenceDecoder as Ref
    assert os.path.realpath(sys.modules[Ref.__module__].__file__).startswith(os.path.realpath(REF))
    from hyena_dna_amd.classifier import SequenceDecoder
    B, L, D = 3, 9, 8
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, L, D, generator=g)
    done = 0
    for d_output in (None, 3):
        for mode, l_out, use_lengths, kw in CASES:
            kw = dict(kw)
            if kw.get("mask") == "prefix":
                n = torch.tensor([4, 9, 1])
                kw["mask"] = (torch.arange(L).unsqueeze(0) < n.unsqueeze(1)).long()
            ours = SequenceDecoder(D, d_output=d_output, l_output=l_out, use_lengths=use_lengths, mode=mode)
            ref = Ref(D, d_output=d_output, l_output=l_out, use_lengths=use_lengths, mode=mode)
            assert list(ours.state_dict()) == list(ref.state_dict()), (mode, list(ours.state_dict()))       # `output_transform.*`
            ref.load_state_dict(ours.state_dict())
            got, want = ours(x, **kw), ref(x, **kw)
            case = (d_output, mode, l_out, use_lengths, sorted(kw))
            assert got.shape == want.shape and got.dtype == want.dtype, (case, got.shape, want.shape)
            assert torch.allclose(got, want, rtol=1e-5, atol=1e-6), (case, (got - want).abs().max().item())
            if d_output is not None:
                assert torch.allclose(ours.step(x[:, 0]), ref.step(x[:, 0]))
            done += 1
    print(f"DECODER_OK cases={done}", flush=True)


if __name__ == "__main__":
    main()
