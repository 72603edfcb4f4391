"""Soft-prompt tuning of a frozen ``HyenaDNALM`` (the reference's in-context-learning experiment: evals/soft_prompting_genomics.py ``LitModel``,
configs/evals/soft_prompting_genomics.yaml): ``n`` learnable fp32 "soft tokens" in front of a few-shot prompt, the loss taken at the label
positions only.

    hidden = backbone(cat([dropout(soft_tokens).expand(B, n, D), embeddings(x)], 1))        LitModel.forward
    logits = lm_head(hidden)[:, n:][:, label_positions - 1]                                 LitModel.step
    loss   = cross_entropy(logits, x[:, label_positions])

Here the soft tokens enter inside the first block's add + LayerNorm pass (``block.soft_embedding_dropout_add_layer_norm``: neither the
(B, L, D) embedding nor the (B, n + L, D) concatenation nor their gradients are stored, the backward reads the B n soft rows only), and the
final norm and the head run on the B n_pos label rows (``HyenaDNALM.hidden_at``) instead of all B (n + L).  The head of this class is the row-wise HIP
head (``row_head``): the logits at the label positions are, bit for bit, the rows of the full-length logits (one exception: ``n_soft_tokens = 0``
without positions is the plain model with its own library-GEMM head, ``SoftPromptLM.forward``).  ``fused=False`` -- or a shape
the kernels do not cover, position embeddings, an unfrozen table / norm1 -- is the reference's statement with ``torch.cat``.

Not covered: ``generate()`` / cached decoding with a soft prefix, and the fused pass with an unfrozen embedding table (that case takes the
unfused route)."""
import torch
import torch.nn as nn

from . import _castcache, _lib
from .lm import token_cross_entropy
from .projection import hyena_linear

__all__ = ["SoftPromptLM", "few_shot_label_positions", "RowHeadFunc", "row_head"]


class RowHeadFunc(torch.autograd.Function):
    """logits = x weight^T on the row-wise HIP head (include/hyena_block.h hyena_row_head_*): every logit is summed in an order that does not depend
    on the number of rows, so the logits of gathered rows are the bits of the same rows of the full-length call.  ``weight`` is frozen: the backward
    returns dx only.  ``dt``: the 16-bit autocast type (``weight`` is then the fp32 parameter, used through its per-step shadow), or None."""

    @staticmethod
    def forward(ctx, x, weight, dt=None):
        w = (weight.detach() if dt is None else _castcache.shadow(weight, dt)).contiguous()
        ctx.save_for_backward(w)
        ctx.shape = x.shape
        return _lib.row_head_fwd(x.reshape(-1, x.shape[-1]).contiguous(), w).view(x.shape[:-1] + (w.shape[0],))

    @staticmethod
    def backward(ctx, dy):
        (w,) = ctx.saved_tensors
        return _lib.row_head_bwd(dy.reshape(-1, w.shape[0]).to(w.dtype).contiguous(), w).view(ctx.shape), None, None


def row_head(x, weight, bias=None):
    """``F.linear(x, weight, bias)`` with nn.Linear's autocast semantics for a FROZEN head of at most 16 classes, row-count invariant bit for bit
    (``RowHeadFunc``); a head the kernel does not cover -- a bias, a weight that wants a gradient, another shape -- goes through ``hyena_linear``"""
    dev_type = x.device.type
    dt = torch.get_autocast_dtype(dev_type) if torch.is_autocast_enabled(dev_type) else None
    if dt not in (torch.bfloat16, torch.float16):
        dt = None
    ct = dt if dt is not None else x.dtype
    if (bias is None and not (torch.is_grad_enabled() and weight.requires_grad) and weight.device == x.device
            and (weight.dtype == ct or (dt is not None and weight.dtype == torch.float32)) and _lib.row_head_supported(weight.shape[0], x.shape[-1], ct)):
        _lib._require_gpu(x, "x")
        with torch.autocast(dev_type, enabled=False):
            return RowHeadFunc.apply(x.to(ct), weight, dt if weight.dtype != ct else None)
    return hyena_linear(x, weight, bias)


def few_shot_label_positions(max_length, total_len):
    """positions of the label tokens in a few-shot sample of ``total_len`` tokens (test label included) whose sequences all have ``max_length``
    tokens: every shot is ``seq + eos + label + eos`` (max_length + 3 tokens), the test sequence ``seq + eos`` is followed by its label --
    ``LitModel.get_labels_idx``: [max_length + 1] + arange(2 max_length + 4, total_len, max_length + 3)"""
    return torch.tensor([max_length + 1] + list(range(2 * max_length + 4, total_len, max_length + 3)), dtype=torch.int64)


class SoftPromptLM(nn.Module):
    """``model`` (a ``HyenaDNALM``, frozen here) with ``n_soft_tokens`` learnable embeddings in front of every input.  ``model`` and ``soft_tokens``
    are named as in the reference's ``LitModel``, so its checkpoints map.  ``n_soft_tokens = 0`` is the plain model (``soft_tokens`` is None).
    ``fused``: take the one-pass first norm where it applies (module docstring)."""

    def __init__(self, model, n_soft_tokens, soft_token_pdrop=0.0, init_std=0.02, fused=True):
        super().__init__()
        if n_soft_tokens < 0:
            raise ValueError(f"n_soft_tokens has to be >= 0, got {n_soft_tokens}")
        if not 0.0 <= soft_token_pdrop < 1.0:
            raise ValueError(f"soft_token_pdrop has to be in [0, 1), got {soft_token_pdrop}")
        self.model = model
        for p in self.model.parameters():                    # only the soft tokens are trained
            p.requires_grad_(False)
        self.n_soft_tokens, self.soft_token_pdrop, self.fused = int(n_soft_tokens), float(soft_token_pdrop), bool(fused)
        if n_soft_tokens > 0:
            w = self.model.lm_head.weight
            self.soft_tokens = nn.Parameter(torch.zeros(n_soft_tokens, w.shape[1], dtype=torch.float32, device=w.device))
            nn.init.normal_(self.soft_tokens, mean=0.0, std=init_std)
        else:
            self.soft_tokens = None

    def forward(self, input_ids, positions=None):
        """logits (B, L, V) of the INPUT positions (the soft positions are never returned), or (B, n_pos, V) at ``positions`` -- an (n_pos,) int64
        index into the input positions, shared by the batch: the final norm and the head then run on those rows only"""
        m = self.model
        if self.soft_tokens is None and positions is None:
            # the plain model itself, its library-GEMM head included: bit for bit ``model(input_ids)`` -- and therefore the one call of this
            # class whose logits are NOT bit for bit the rows ``forward(input_ids, positions)`` returns (row-wise head); they agree to the
            # head's rounding (1 - 2 ulp)
            return m(input_ids)[0].logits
        if positions is None:
            # norm and head over the n + L rows as they lie, the logits sliced: no (B, L, D) copy to cut the soft rows out
            hidden, n = m._hidden_all(input_ids, self.soft_tokens, self.soft_token_pdrop, self.fused)
            return row_head(hidden, m.lm_head.weight, m.lm_head.bias)[:, n:n + input_ids.shape[1]]
        hidden = m.hidden_at(input_ids, positions, soft_tokens=self.soft_tokens, soft_dropout_p=self.soft_token_pdrop, soft_fused=self.fused)
        return row_head(hidden, m.lm_head.weight, m.lm_head.bias)

    def loss(self, input_ids, label_positions, return_logits=False):
        """``LitModel.step``: the logits at ``label_positions - 1`` predict ``input_ids[:, label_positions]``; mean cross entropy over B n_pos"""
        label_positions = torch.as_tensor(label_positions, dtype=torch.int64, device=input_ids.device).reshape(-1)
        logits = self.forward(input_ids, label_positions - 1)
        loss = token_cross_entropy(logits, input_ids[:, label_positions])
        return (loss, logits) if return_logits else loss

    @torch.no_grad()
    def predict(self, input_ids):
        """the argmax token after the last input position, (B,)"""
        last = torch.tensor([input_ids.shape[1] - 1], dtype=torch.int64, device=input_ids.device)
        return self.forward(input_ids, last)[:, 0].argmax(-1)
