"""Sequence-level classification / regression on top of the HyenaDNA backbone: the third thing people do with the model besides
pre-training (``runner.py``, ``lm.HyenaDNALM``) and generation.

What the reference does here, restated:

* ``DNAEmbeddingModel`` (src/models/sequence/dna_embedding.py): the pre-training model without its head in the forward -- same modules and
  state-dict names, the tied ``lm_head`` included, so a pre-training checkpoint loads -- returning the hidden states of the final norm;
* ``SequenceDecoder`` (src/tasks/decoders.py): picks ``l_output`` positions of the hidden states (``last`` / ``first``) or reduces over the
  sequence (``pool``: running mean, ``sum``: running sum), then a linear ``output_transform``;
* ``load_backbone`` (dna_embedding.py): a pre-training state dict -> the fine-tuning model, heads and decoders kept fresh.

What is different: ``HyenaDNAClassifier`` joins the two so that a pooled readout never sees a normalised (B, L, D) tensor.  The reference runs
``ln_f`` over all positions, then ``cumsum / arange`` over the result and keeps one row; here the backbone stops in front of ``drop_f`` /
``ln_f`` (``HyenaDNALM.trunk``) and ``block.dropout_add_layer_norm_pool`` normalises and reduces in one pass over ``(hidden, residual)``, forward
and backward (csrc/block_kernels.h).  ``last`` / ``first`` slice the rows they want BEFORE the final norm.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .block import dropout_add_layer_norm, dropout_add_layer_norm_pool, masked_pool
from .lm import HyenaDNALM, token_cross_entropy

__all__ = ["DNAEmbeddingModel", "SequenceDecoder", "HyenaDNAClassifier", "load_backbone"]


class DNAEmbeddingModel(HyenaDNALM):
    """``HyenaDNALM`` whose forward stops at the hidden states of the final norm: ``forward(...) -> (hidden (B, L, D), None)``."""

    def __init__(self, *args, return_hidden_state=False, **kwargs):
        super().__init__(*args, **kwargs)
        self.return_hidden_state = return_hidden_state        # (kept, as the reference keeps it: nothing reads it)

    def forward(self, input_ids, position_ids=None, inference_params=None, state=None):
        if inference_params is not None or position_ids is not None:
            return self.hidden(input_ids, position_ids, inference_params=inference_params), None
        L = input_ids.shape[1]
        Lp = self._aligned_length(input_ids)
        if Lp != L:
            input_ids = F.pad(input_ids, (0, Lp - L), value=0)
        hidden = self.hidden(input_ids)
        return (hidden[:, :L] if Lp != L else hidden), None

    @property
    def d_output(self):
        return self.d_model


class SequenceDecoder(nn.Module):
    """(B, L, d_model) hidden states -> (B, l_output, d_output), or (B, d_output) with ``l_output=0``.

    ``mode``: ``last`` / ``first`` -- the last / first ``l_output`` positions; ``pool`` / ``sum`` -- the mean / sum over the sequence, one output
    position.  ``use_lengths``: sequence b is its first ``lengths[b]`` positions.  ``mask`` (pool): sequence b is its first ``mask[b].sum()``
    positions.  Reductions are taken in fp32.  The reference's ``ragged`` mode and a pooled readout at more than one position (its running mean at
    each of the last ``l_output`` positions) are refused."""

    def __init__(self, d_model, d_output=None, l_output=None, use_lengths=False, mode="last"):
        super().__init__()
        if mode == "ragged":
            raise NotImplementedError("SequenceDecoder: mode 'ragged' is not supported")
        if mode not in ("last", "first", "pool", "sum"):
            raise NotImplementedError("SequenceDecoder: mode has to be one of 'last', 'first', 'pool', 'sum'")
        self.output_transform = nn.Identity() if d_output is None else nn.Linear(d_model, d_output)
        if l_output is None:
            self.l_output, self.squeeze = None, False
        elif l_output == 0:
            self.l_output, self.squeeze = 1, True
        else:
            if l_output < 0:
                raise ValueError("l_output has to be >= 0")
            self.l_output, self.squeeze = l_output, False
        self.use_lengths = use_lengths
        self.mode = mode

    def positions(self, L, l_output=None):
        """(number of output positions, squeeze?) for hidden states of L positions"""
        if self.l_output is not None:
            return self.l_output, self.squeeze
        if l_output is not None:
            if not isinstance(l_output, int):
                raise TypeError("l_output has to be an int")
            return l_output, False
        return L, False

    def readout(self, x, lengths=None, l_output=None, mask=None, use_lengths=None):
        """everything but the output transform: (B, L, D) -> (B, l, D), or (B, D) when squeezed"""
        B, L, D = x.shape
        l, squeeze = self.positions(L, l_output)
        use_lengths = self.use_lengths if use_lengths is None else use_lengths
        if use_lengths and lengths is None:
            raise ValueError("SequenceDecoder: use_lengths needs `lengths`")
        n = None
        if use_lengths:
            n = torch.as_tensor(lengths, device=x.device).to(torch.long)
        if self.mode in ("pool", "sum"):
            if self.mode == "pool" and mask is not None:
                if use_lengths:
                    raise NotImplementedError("SequenceDecoder: `mask` together with use_lengths")
                n = mask.sum(-1).reshape(B).to(torch.long)
            elif l != 1:
                raise NotImplementedError(f"SequenceDecoder: mode {self.mode!r} with {l} output positions (one pooled position only)")
            y = masked_pool(x, n, "mean" if self.mode == "pool" else "sum").to(x.dtype).unsqueeze(1)
        elif n is None:
            y = x[:, L - l:] if self.mode == "last" else x[:, :l]
        else:
            first = (n - l) if self.mode == "last" else torch.zeros_like(n)
            idx = (first.unsqueeze(1) + torch.arange(l, device=x.device).unsqueeze(0)).clamp(0, L - 1)
            y = x.gather(1, idx.unsqueeze(-1).expand(B, l, D))
        if squeeze:
            assert y.shape[1] == 1
            y = y.squeeze(1)
        return y

    def forward(self, x, state=None, lengths=None, l_output=None, mask=None):
        return self.output_transform(self.readout(x, lengths=lengths, l_output=l_output, mask=mask))

    def step(self, x, state=None):
        return self.output_transform(x)


class HyenaDNAClassifier(nn.Module):
    """``backbone`` (a ``DNAEmbeddingModel``) + ``decoder`` (a ``SequenceDecoder`` with one output position): ``forward(input_ids, lengths=None)
    -> (B, d_output)`` fp32 (``(B, 1, d_output)`` if the decoder does not squeeze).

    ``lengths`` (B,): sequence b is its first ``lengths[b]`` tokens (END-padded batches); with ``pad_token_id`` set and no ``lengths`` given they
    are counted on the device as the tokens that are not pads -- so a captured step (``lm.GraphedTrainStep``, which hands over ids and labels
    only) serves variable-length batches.  ``fused_readout=False`` takes the unfused route (final norm over all positions, then the reduction):
    the same graph, kept selectable for comparisons."""

    def __init__(self, backbone, decoder, pad_token_id=None, fused_readout=True):
        super().__init__()
        self.backbone, self.decoder = backbone, decoder
        self.pad_token_id, self.fused_readout = pad_token_id, fused_readout

    def _head(self, y):
        dev = y.device.type
        with torch.autocast(dev, enabled=False):               # the output transform in fp32 on the fp32 readout
            return self.decoder.output_transform(y.float())

    def _fused_pool_ok(self, hidden_states):
        bb = self.backbone
        ln = bb.backbone.ln_f
        from . import _lib
        return (self.fused_readout and bb.fused_dropout_add_ln and bb.residual_in_fp32 and ln.weight is not None
                and (hidden_states.is_cuda or _lib._backend.name != "hip")
                and _lib.add_norm_pool_supported(hidden_states.shape[-1], hidden_states.dtype))

    def forward(self, input_ids, lengths=None):
        bb, dec = self.backbone, self.decoder
        B, L = input_ids.shape
        l, squeeze = dec.positions(L)
        if l != 1:
            raise NotImplementedError("HyenaDNAClassifier reads one output position (SequenceDecoder l_output 0 or 1)")
        if lengths is None and self.pad_token_id is not None:
            lengths = (input_ids != self.pad_token_id).sum(-1)
        if lengths is not None:
            lengths = torch.as_tensor(lengths, device=input_ids.device).clamp(0, L)
        Lp = bb._aligned_length(input_ids)
        if Lp != L:
            input_ids = F.pad(input_ids, (0, Lp - L), value=0)      # causal stack: positions < L see what the unpadded run shows them
        hidden_states, residual = bb.trunk(input_ids)
        ln, p = bb.backbone.ln_f, (bb.backbone.drop_f.p if self.training else 0.0)
        if dec.mode in ("pool", "sum"):
            if lengths is None and Lp != L:
                lengths = torch.full((B,), L, dtype=torch.int32, device=input_ids.device)      # the pad positions are never pooled
            if self._fused_pool_ok(hidden_states):
                y = dropout_add_layer_norm_pool(hidden_states, residual, ln.weight, ln.bias, p, ln.eps, lengths=lengths,
                                                mode="mean" if dec.mode == "pool" else "sum", residual_in_fp32=True)
            else:
                y = masked_pool(bb._final_norm(hidden_states, residual), lengths, "mean" if dec.mode == "pool" else "sum")
        else:
            # last / first: one row per sequence goes through the final norm
            if dec.mode == "first":
                idx = torch.zeros(B, dtype=torch.long, device=input_ids.device)
            elif lengths is None:
                idx = torch.full((B,), L - 1, dtype=torch.long, device=input_ids.device)
            else:
                idx = (lengths.to(torch.long) - 1).clamp_min(0)
            D = hidden_states.shape[-1]
            take = idx.view(B, 1, 1).expand(B, 1, D)
            h1 = hidden_states.gather(1, take)
            r1 = None if residual is None else residual.gather(1, take)
            y = bb._final_norm(h1, r1).squeeze(1).float()
        y = self._head(y)
        return y if squeeze else y.unsqueeze(1)

    def loss(self, input_ids, targets, ignore_index=-100):
        """cross entropy over the classes (the reference's ``multiclass`` tasks: src/tasks/metrics.py cross_entropy), labels (B,)"""
        logits = self.forward(input_ids)
        return token_cross_entropy(logits.reshape(targets.numel(), -1), targets, ignore_index=ignore_index)


def load_backbone(model, state_dict, freeze_backbone=False, ignore_head=True):
    """A pre-training checkpoint -> ``model`` (a ``DNAEmbeddingModel``, or a ``HyenaDNAClassifier``: its backbone), in place.

    A leading ``model.`` is stripped from the checkpoint's keys.  Every key of the model has to be in the checkpoint (``KeyError`` otherwise),
    except that keys containing ``decoder`` -- and, with ``ignore_head``, keys containing ``head`` -- keep the model's fresh values whether the
    checkpoint has them or not.  (``lm_head.weight`` is tied to the token embedding, which IS loaded.)  ``freeze_backbone``: the backbone's
    parameters stop requiring gradients; a classifier's decoder stays trainable.  Returns the state dict that was loaded."""
    target = model.backbone if isinstance(model, HyenaDNAClassifier) else model
    sd = {(k[len("model."):] if k.startswith("model.") else k): v for k, v in state_dict.items()}
    own = target.state_dict()
    used = {}
    for key in sorted(own):
        if "decoder" in key or (ignore_head and "head" in key):
            used[key] = own[key]
        elif key not in sd:
            raise KeyError(f"load_backbone: {key!r} is missing from the checkpoint")
        else:
            used[key] = sd[key]
    target.load_state_dict(used, strict=True)
    if hasattr(target, "tie_weights"):
        target.tie_weights()
    if freeze_backbone:
        for p in target.parameters():
            p.requires_grad = False
    return used
