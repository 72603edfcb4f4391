"""Model glue around the Hyena mixer, MI355X-side: what the reference's backbone imports from ``flash_attn``
(``src/models/sequence/long_conv_lm.py:18-33``) and, on top of it, a Lightning-free language model of the same structure.

The reference's ``ConvLMHeadModel`` (``long_conv_lm.py:400-502``) is built from flash_attn's ``GPT2Embeddings``,
``Block``, ``Mlp``, ``MHA`` and ``GenerationMixin`` -- CUDA-only in the pinned flash_attn, and restated in plain PyTorch
by the reference itself at ``src/models/sequence/simple_lm.py:26-305`` / ``standalone_hyenadna.py:302-561``.  The classes
below follow those restatements' semantics (same constructor arguments, attribute / state-dict names and forward
contracts), so that the unmodified reference backbone builds on ROCm once ``overlay/flash_attn`` (thin re-exports of
this module) is on ``sys.path`` -- INTEGRATION.md section 4.  What is MI355X-specific:

* ``Block`` routes its two (dropout ->) add -> LayerNorm steps through the fused HIP kernels of
  ``hyena_dna_amd.block.dropout_add_layer_norm`` when ``fused_dropout_add_ln=True``;
* ``Mlp`` (tanh-GELU, ``long_conv_lm.py:117-123``) runs its two products that contract over d_model on this package's
  weights-stationary MFMA kernels with the element-wise passes in their epilogues (``FusedMlpFunc``: fc1 + bias + GELU forward,
  (dy W2) * GELU' + bias-gradient sums backward; ``csrc/proj_kernels.h``); fc2, the input gradient and the weight gradients
  stay library GEMMs, the latter with the split-K schedule of ``hyena_dna_amd.projection``;
* the mixer is whatever ``mixer_cls`` builds -- ``hyena_dna_amd.hyena.HyenaOperator`` through the registry swap.

``HyenaDNALM`` = embedding -> n_layer x Block -> (dropout, add,) LayerNorm -> tied LM head, the hyenadna-* model family
(``hg38_hyena.yaml``), with ``loss()`` = next-token cross entropy: the full-model step ``bench.py`` times as a secondary
figure (north_star configuration 5).
"""
import math
import os
from collections import namedtuple
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

from .block import dropout_add_layer_norm, embedding_dropout_add_layer_norm, embedding_fusable, soft_embedding_dropout_add_layer_norm
from .projection import hyena_linear

__all__ = ["Mlp", "Block", "GPT2Embeddings", "MHA", "GenerationMixin", "HyenaDNALM", "GraphedDecodeStep", "sync_shared_params", "all_gather_raw"]


# ---------------------------------------------------------------------------------------------------------------------
# flash_attn.modules.mlp.Mlp  (semantics: simple_lm.py:192-212)
# ---------------------------------------------------------------------------------------------------------------------
class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, activation=F.gelu, return_residual=False,
                 device=None, dtype=None):
        factory_kwargs = {"device": device, "dtype": dtype}
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.return_residual = return_residual
        self.fc1 = nn.Linear(in_features, hidden_features, **factory_kwargs)
        self.activation = activation
        self.fc2 = nn.Linear(hidden_features, out_features, **factory_kwargs)

    def forward(self, x):
        if self._fused_ok(x):
            y = fused_mlp(x, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias)
        else:
            y = hyena_linear(x, self.fc1.weight, self.fc1.bias)
            y = self.activation(y)
            y = hyena_linear(y, self.fc2.weight, self.fc2.bias)
        return y if not self.return_residual else (y, x)

    def _fused_ok(self, x):
        """The matrix-core MLP kernels (csrc/proj_kernels.h) cover the HyenaDNA block: tanh-GELU, 16-bit compute (autocast or
        plain), d_model 128 / 256, d_inner a multiple of 256, biases present."""
        act = self.activation
        tanh_gelu = (isinstance(act, partial) and act.func is F.gelu and act.keywords.get("approximate") == "tanh" and not act.args)
        if not (FUSED_MLP and tanh_gelu and self.fc1.bias is not None and self.fc2.bias is not None):
            return False
        from . import _lib
        if not (x.is_cuda or _lib._backend.name != "hip"):
            return False
        dt = _mlp_dtype(x, self.fc1.weight)
        rows = x.numel() // max(x.shape[-1], 1)
        # fc1's kernel contracts over in_features, the fused backward (`mlp_dh_dgelu_bwd`) over fc2.out_features: both must be a width the
        # kernels are built for, whatever `out_features` the caller chose (the reference's Mlp accepts any; other widths take the library path)
        return (dt is not None and rows >= 1 and self.fc2.in_features == self.fc1.out_features
                and _lib.mlp_supported(rows, self.fc1.in_features, self.fc1.out_features, dt)
                and _lib.mlp_supported(rows, self.fc2.out_features, self.fc1.out_features, dt))


FUSED_MLP = os.environ.get("HYENA_FUSED_MLP", "1") != "0"          # A/B knob: 0 = two library GEMMs + PyTorch's GELU
# HyenaDNALM pads batches of several odd-length sequences to a multiple of 64 positions (HyenaDNALM._aligned_length); 0 = run them as they come
PAD_SEQUENCES = os.environ.get("HYENA_LM_PAD_SEQUENCES", "1") != "0"
_SEQ_ALIGN = 64
_PAD_SINGLE_MIN = int(os.environ.get("HYENA_LM_PAD_SINGLE_MIN", "8192"))      # a single sequence is padded from this length on (_aligned_length) ...
_PAD_SINGLE_ROWS = 4096                                                        # ... if the padded length is a multiple of this (64 weight-gradient slices of 64-aligned rows)


def _mlp_dtype(x, weight):
    if torch.is_autocast_enabled():
        dt = torch.get_autocast_dtype("cuda" if x.is_cuda else "cpu")
        return dt if dt in (torch.bfloat16, torch.float16) else None
    return x.dtype if x.dtype in (torch.bfloat16, torch.float16) and weight.dtype == x.dtype else None


class FusedMlpFunc(torch.autograd.Function):
    """y = fc2(gelu_tanh(fc1(x))) (simple_lm.py:207-211) with the element-wise passes inside this package's MFMA kernels:

        forward   a, h = mlp_fc1_gelu_fwd(x, W1, b1)          one launch: a = x W1^T + b1 and h = gelu(a), both kept (a for the
                  y = h W2^T + b2                              backward, h as fc2's operand -- what autograd keeps today as well)
        backward  da, db1 = mlp_dh_dgelu_bwd(dy, W2^T, a)      one launch: (dy W2) * gelu'(a) and its column sums
                  dx = da W1;  dW1 = da^T x;  dW2 = dy^T h;  db2 = sum dy        library GEMMs (contractions over d_inner / positions)

    Gone: the GELU pass (read a, write h), the GELU-backward pass (read a, dh, write da), the dh tensor and fc1's bias-gradient
    reduction -- 12 of the ~28 GB a layer's MLP moves at L = 2^20."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, dt=None):
        # dt: autocast's compute type -- w1 ... b2 are then the fp32 PARAMETERS, used through their per-step shadows (_castcache: one batched cast
        # per optimizer step), and their gradients go back in fp32; None: operands already in the compute type
        from . import _castcache, _lib
        ctx.ptypes = (w1.dtype, b1.dtype, w2.dtype, b2.dtype, dt)
        if dt is not None:
            b1f = _castcache.rounded_f32(b1, dt)                             # b1 rounded to the compute type (autocast semantics), in fp32
            w1, w2, b2 = _castcache.shadow(w1, dt), _castcache.shadow(w2, dt), _castcache.shadow(b2, dt)
        else:
            b1f = b1.float().contiguous()
        x2 = x.reshape(-1, x.shape[-1])
        a, h = _lib.mlp_fc1_gelu_fwd(x2, w1, b1f)
        y = torch.addmm(b2, h, w2.t())
        ctx.save_for_backward(x2, w1, w2, a, h)
        ctx.xshape = x.shape
        return y.view(*x.shape[:-1], w2.shape[0])

    @staticmethod
    def backward(ctx, dy):
        from . import _castcache, _lib
        from .projection import split_k_weight_grad
        x2, w1, w2, a, h = ctx.saved_tensors
        t_w1, t_b1, t_w2, t_b2, dt = ctx.ptypes
        cdt = dt if dt is not None else dy.dtype
        dy2 = dy.reshape(-1, dy.shape[-1]).contiguous()
        da, db1 = _lib.mlp_dh_dgelu_bwd(dy2, w2.t().contiguous(), a)
        dx = dw1 = dw2 = db2 = None
        if ctx.needs_input_grad[0]:
            dx = torch.mm(da, w1).view(ctx.xshape)
        if ctx.needs_input_grad[1]:
            dw1 = _castcache.wgrad_out(split_k_weight_grad(da, x2), t_w1, cdt)
        if ctx.needs_input_grad[3]:
            dw2 = _castcache.wgrad_out(split_k_weight_grad(dy2, h), t_w2, cdt)
        if ctx.needs_input_grad[4]:
            db2 = _castcache.wgrad_out(_lib.colsum(dy2), t_b2, cdt)
        return dx, dw1, _castcache.wgrad_out(db1, t_b1, cdt) if ctx.needs_input_grad[2] else None, dw2, db2, None


def fused_mlp(x, w1, b1, w2, b2):
    dt = _mlp_dtype(x, w1)
    with torch.autocast("cuda" if x.is_cuda else "cpu", enabled=False):
        if all(t.dtype == torch.float32 for t in (w1, b1, w2, b2)):        # autocast over fp32 parameters: through their per-step shadows
            return FusedMlpFunc.apply(x.to(dt).contiguous(), w1, b1, w2, b2, dt)
        return FusedMlpFunc.apply(x.to(dt).contiguous(), w1.to(dt).contiguous(), b1.to(dt), w2.to(dt).contiguous(), b2.to(dt))


def _refuse(name):
    class _Missing(nn.Module):
        def __init__(self, *a, **k):
            raise NotImplementedError(f"flash_attn.{name} (tensor / sequence parallel or fused-dense variants) is not part of the "
                                      "HyenaDNA path: every hg38 configuration builds the plain module (process_group=None)")
    _Missing.__name__ = name.rsplit(".", 1)[-1]
    return _Missing


FusedMLP = _refuse("modules.mlp.FusedMLP")
ParallelFusedMLP = _refuse("modules.mlp.ParallelFusedMLP")
ParallelMHA = _refuse("modules.mha.ParallelMHA")
ParallelGPT2Embeddings = _refuse("modules.embedding.ParallelGPT2Embeddings")


# ---------------------------------------------------------------------------------------------------------------------
# flash_attn.modules.mha.MHA  (semantics: simple_lm.py:26-150; HyenaDNA sets attn_layer_idx = None, so this is only
# ever built by hybrid configurations)
# ---------------------------------------------------------------------------------------------------------------------
class MHA(nn.Module):
    def __init__(self, embed_dim, num_heads, bias=True, dropout=0.0, softmax_scale=None, causal=False, layer_idx=None,
                 dwconv=False, return_residual=False, device=None, dtype=None, **unused):
        factory_kwargs = {"device": device, "dtype": dtype}
        super().__init__()
        assert embed_dim % num_heads == 0, "self.kdim must be divisible by num_heads"
        self.embed_dim, self.num_heads, self.head_dim = embed_dim, num_heads, embed_dim // num_heads
        self.causal, self.layer_idx, self.dwconv, self.return_residual = causal, layer_idx, dwconv, return_residual
        self.softmax_scale, self.dropout_p = softmax_scale, dropout
        self.Wqkv = nn.Linear(embed_dim, 3 * embed_dim, bias=bias, **factory_kwargs)
        if dwconv:
            self.dwconv_qkv = nn.Conv1d(3 * embed_dim, 3 * embed_dim, kernel_size=3, padding=2, groups=3 * embed_dim)
        self.out_proj = nn.Linear(embed_dim, embed_dim, **factory_kwargs)

    def forward(self, x, key_padding_mask=None, **kwargs):
        qkv = self.Wqkv(x)
        if self.dwconv:
            qkv = self.dwconv_qkv(qkv.transpose(1, 2))[..., :-2].transpose(1, 2).contiguous()
        B, S, _ = qkv.shape
        q, k, v = qkv.view(B, S, 3, self.num_heads, self.head_dim).permute(2, 0, 3, 1, 4)      # (3, B, H, S, d)
        mask = None
        if key_padding_mask is not None:
            mask = key_padding_mask[:, None, None, :]
            if self.causal:
                mask = mask & torch.ones(S, S, dtype=torch.bool, device=x.device).tril()
        ctx = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, dropout_p=self.dropout_p if self.training else 0.0,
                                             is_causal=self.causal and mask is None, scale=self.softmax_scale)
        out = self.out_proj(ctx.transpose(1, 2).reshape(B, S, self.embed_dim))
        return out if not self.return_residual else (out, x)


# ---------------------------------------------------------------------------------------------------------------------
# flash_attn.modules.embedding.GPT2Embeddings  (semantics: simple_lm.py:153-190)
# ---------------------------------------------------------------------------------------------------------------------
class SmallVocabEmbeddingFunc(torch.autograd.Function):
    """``F.embedding`` whose weight gradient is a dense product ``onehot(ids)^T @ dh``.  PyTorch's embedding backward sorts /
    scatters per token; with the 16-row DNA vocabulary and 10^6 tokens per sequence every token collides with 2.6e5 others
    and that kernel alone took 10.5 ms of a 212 ms model step (profiles/r2h).  The one-hot product is one slice-batched
    GEMM (``projection.split_k_weight_grad``), deterministic."""

    @staticmethod
    def forward(ctx, ids, weight):
        ctx.save_for_backward(ids)
        ctx.vocab = weight.shape[0]
        return F.embedding(ids, weight)

    @staticmethod
    def backward(ctx, dh):
        from .projection import split_k_weight_grad
        (ids,) = ctx.saved_tensors
        dh2 = dh.reshape(-1, dh.shape[-1]).contiguous()               # (whatever layout dh arrives in: the same product, the same bits)
        onehot = F.one_hot(ids.reshape(-1), ctx.vocab).to(dh2.dtype)
        return None, split_k_weight_grad(onehot, dh2).to(dh.dtype)


def small_vocab_embedding(ids, emb):
    if (ids.is_cuda and emb.padding_idx is None and emb.max_norm is None and not emb.sparse and emb.num_embeddings <= 64
            and ids.numel() >= 32768):
        return SmallVocabEmbeddingFunc.apply(ids, emb.weight)
    return emb(ids)


class GPT2Embeddings(nn.Module):
    def __init__(self, embed_dim, vocab_size, max_position_embeddings, padding_idx=None, word_embed_proj_dim=None,
                 device=None, dtype=None):
        factory_kwargs = {"device": device, "dtype": dtype}
        super().__init__()
        if word_embed_proj_dim is None:
            self.word_embeddings = nn.Embedding(vocab_size, embed_dim, padding_idx=padding_idx, **factory_kwargs)
            self.project_in = None
        else:
            self.word_embeddings = nn.Embedding(vocab_size, word_embed_proj_dim, padding_idx=padding_idx, **factory_kwargs)
            self.project_in = nn.Linear(word_embed_proj_dim, embed_dim, bias=False, **factory_kwargs)
        self.max_position_embeddings = max_position_embeddings
        if self.max_position_embeddings > 0:
            self.position_embeddings = nn.Embedding(max_position_embeddings, embed_dim, **factory_kwargs)

    def forward(self, input_ids, position_ids=None):
        batch_size, seqlen = input_ids.shape
        embeddings = small_vocab_embedding(input_ids, self.word_embeddings)
        if self.project_in is not None:
            embeddings = self.project_in(embeddings)
        if self.max_position_embeddings > 0:
            if position_ids is None:
                position_ids = torch.arange(seqlen, dtype=torch.long, device=input_ids.device)
            embeddings = embeddings + self.position_embeddings(position_ids)
        return embeddings


# ---------------------------------------------------------------------------------------------------------------------
# flash_attn.modules.block.Block  (semantics: simple_lm.py:214-305; constructor as long_conv_lm.py:171-185 calls it)
# ---------------------------------------------------------------------------------------------------------------------
class Block(nn.Module):
    def __init__(self, dim, mixer_cls=None, mlp_cls=None, norm_cls=nn.LayerNorm, dropout_cls=nn.Dropout, prenorm=True,
                 resid_dropout1=0.0, resid_dropout2=0.0, drop_path1=0.0, drop_path2=0.0, fused_dropout_add_ln=False,
                 return_residual=False, residual_in_fp32=False, sequence_parallel=False, mark_shared_params=False):
        super().__init__()
        if drop_path1 or drop_path2:
            raise NotImplementedError("stochastic depth is not used by any HyenaDNA configuration")
        if sequence_parallel or mark_shared_params:
            raise NotImplementedError("tensor / sequence parallelism is not part of the HyenaDNA path (north_star: data parallel only)")
        self.prenorm = prenorm
        self.fused_dropout_add_ln = fused_dropout_add_ln
        self.return_residual = return_residual
        self.residual_in_fp32 = residual_in_fp32
        if self.residual_in_fp32:
            assert self.prenorm, "residual_in_fp32 is only compatible with prenorm=True"
        if mixer_cls is None:
            mixer_cls = partial(MHA, num_heads=dim // 64)
        if mlp_cls is None:
            mlp_cls = partial(Mlp, hidden_features=4 * dim)
        self.mixer = mixer_cls(dim)
        self.dropout1 = dropout_cls(resid_dropout1)
        self.norm1 = norm_cls(dim)
        self.mlp = mlp_cls(dim)
        if not isinstance(self.mlp, nn.Identity):
            self.dropout2 = dropout_cls(resid_dropout2)
            self.norm2 = norm_cls(dim)

    def _add_norm(self, hidden_states, residual, drop, norm):
        if self.fused_dropout_add_ln:
            return dropout_add_layer_norm(hidden_states, residual, norm.weight, norm.bias, drop.p if self.training else 0.0,
                                          norm.eps, prenorm=True, residual_in_fp32=self.residual_in_fp32)
        dropped = drop(hidden_states)
        residual = (dropped + residual) if residual is not None else dropped
        hidden_states = norm(residual.to(dtype=norm.weight.dtype))
        if self.residual_in_fp32:
            residual = residual.to(torch.float32)
        return hidden_states, residual

    def forward(self, hidden_states, residual=None, mixer_subset=None, mixer_kwargs=None, normed=False):
        """``normed``: (hidden_states, residual) are already the outputs of this block's first dropout -> add -> LayerNorm (HyenaDNALM hands
        them over when that pass also gathered the token embedding)"""
        if self.prenorm:
            if not normed:
                hidden_states, residual = self._add_norm(hidden_states, residual, self.dropout1, self.norm1)
            mixer_kwargs = {} if mixer_kwargs is None else mixer_kwargs
            if mixer_subset is not None:
                mixer_kwargs["mixer_subset"] = mixer_subset
            fused = None
            if (not mixer_kwargs and not isinstance(self.mlp, nn.Identity) and self.fused_dropout_add_ln and self.residual_in_fp32
                    and (self.dropout2.p == 0.0 or not self.training) and hasattr(self.mixer, "forward_add_norm")
                    and isinstance(self.norm2, nn.LayerNorm) and self.norm2.weight is not None):
                # the mixer's last kernel carries this block's second add + LayerNorm in its epilogue (hyena.HyenaOperator.forward_add_norm)
                fused = self.mixer.forward_add_norm(hidden_states, residual, self.norm2.weight, self.norm2.bias, self.norm2.eps)
            if fused is not None:
                hidden_states, residual = fused
                return self.mlp(hidden_states), residual
            hidden_states = self.mixer(hidden_states, **mixer_kwargs)
            if mixer_subset is not None:
                residual = residual[:, mixer_subset]
            if not isinstance(self.mlp, nn.Identity):
                hidden_states, residual = self._add_norm(hidden_states, residual, self.dropout2, self.norm2)
                hidden_states = self.mlp(hidden_states)
            return hidden_states, residual
        assert residual is None
        mixer_out = self.mixer(hidden_states, **(mixer_kwargs if mixer_kwargs is not None else {}))
        if self.return_residual:
            mixer_out, hidden_states = mixer_out
        hidden_states = self.norm1((self.dropout1(mixer_out) + hidden_states).to(dtype=self.norm1.weight.dtype))
        if not isinstance(self.mlp, nn.Identity):
            mlp_out = self.mlp(hidden_states)
            if self.return_residual:
                mlp_out, hidden_states = mlp_out
            hidden_states = self.norm2((self.dropout2(mlp_out) + hidden_states).to(dtype=self.norm2.weight.dtype))
        return hidden_states


# ---------------------------------------------------------------------------------------------------------------------
# flash_attn.utils.generation.GenerationMixin / flash_attn.utils.distributed
# ---------------------------------------------------------------------------------------------------------------------
def _last_logits(out):
    logits = (out[0] if isinstance(out, tuple) else out)
    return (logits.logits if hasattr(logits, "logits") else logits)[:, -1]


def _sample(logits, top_k, temperature):
    logits = logits / max(temperature, 1e-6)
    if top_k <= 1:
        nxt = logits.argmax(-1, keepdim=True)
    else:
        v, i = logits.topk(top_k, dim=-1)
        nxt = i.gather(-1, torch.multinomial(torch.softmax(v.float(), -1), 1))
    return logits, nxt


def _allowed_masks(allowed_tokens, constraints, min_new_tokens, eos_token_id, G, fan, N, dev):
    """generate()'s ``allowed_tokens`` / ``constraints`` / ``min_new_tokens`` as the device sampler's masks -> (allow, check): ``allow`` None
    where none is given, else int64 (N,) or (G fan, N) on ``dev``, their intersection; ``check(V, Vlive)`` raises for an id outside [0, V)
    and for a position that allows no token below ``Vlive`` (named by row and position).  A wrong shape, dtype or device is refused here.
    The one read-back -- the highest lowest-set-bit over the masks, and where it stands -- is made HERE, before the prefill is launched
    (the host then waits for next to nothing); ``check`` compares host numbers once the prefill's logits have told V."""
    from .inference import token_mask
    m = int(min_new_tokens)
    if m < 0:
        raise ValueError(f"min_new_tokens={min_new_tokens}: a number of tokens")
    if m and eos_token_id is None:
        raise ValueError("min_new_tokens keeps eos_token_id out of the first positions: it needs eos_token_id")
    if allowed_tokens is None and constraints is None and not m:
        return None, lambda V, Vlive: None
    ids = None if allowed_tokens is None else [int(v) for v in allowed_tokens]
    keep = -1 if ids is None else token_mask(v for v in ids if 0 <= v < 64)      # (an id outside: check() names it)
    if constraints is None:
        allow = torch.full((N,), keep, dtype=torch.int64, device=dev)
    else:
        ok = torch.is_tensor(constraints) and constraints.dtype == torch.int64 and constraints.device == dev
        if not ok or tuple(constraints.shape) not in ((N,), (G, N)):
            what = f"{tuple(constraints.shape)} {constraints.dtype} on {constraints.device}" if torch.is_tensor(constraints) else type(constraints).__name__
            raise ValueError(f"constraints must be a ({N},) or ({G}, {N}) int64 tensor of bit masks on {dev}, N = max_length - the prompt's "
                             f"columns (got {what})")
        allow = constraints & keep
        if allow.dim() == 2 and fan > 1:
            allow = allow.repeat_interleave(fan, 0)
    if m and 0 <= int(eos_token_id) < 64:
        allow = allow.clone()
        allow[..., :m] &= ~token_mask([eos_token_id])
    allow = allow.contiguous()
    flat = allow.reshape(-1)
    pow2 = torch.ones(64, dtype=torch.int64, device=dev) << torch.arange(64, device=dev)
    low = torch.where(flat == 0, 64, ((flat & -flat)[:, None] == pow2[None]).int().argmax(1))       # lowest set bit; 64: no bit at all
    worst, at = torch.stack([low.max(), low.argmax()]).tolist()                                       # the one host read

    def check(V, Vlive):
        bad = [v for v in ids or () if not 0 <= v < V]
        if bad:
            raise ValueError(f"allowed_tokens holds {bad[0]}: the logits have {V} columns")
        if m and not 0 <= int(eos_token_id) < V:
            raise ValueError(f"eos_token_id={eos_token_id}: the logits have {V} columns")
        if worst >= Vlive:
            where = f"position {at}" if allow.dim() == 1 else f"row {at // N}, position {at % N}"
            raise ValueError(f"the constraints allow no token below {Vlive} (the live vocabulary) at {where}")
    return allow, check


def _automaton_tables(automaton, input_ids, lengths, fan, N, V, vocab_size, allowed_tokens, constraints, min_new_tokens, eos_token_id):
    """generate()'s ``automaton`` as the tables of the device sampler / beam searcher -> (M (Nt, S) int64, delta (S, V) int32, dstate
    (G fan,) int32) on the input's device.  Everything that can be refused is refused here, before a cache exists: per-row positional masks,
    an automaton over another alphabet than the logits', a table over the limit, a row whose prompt leaves no accepted continuation.  One
    read-back: the last ``context`` prompt tokens of every row (and the positional masks, where there are any)."""
    from .inference import TokenAutomaton, automaton_step_tables
    A, dev = automaton, input_ids.device
    if not isinstance(A, TokenAutomaton):
        raise ValueError(f"automaton must be an inference.TokenAutomaton (got {type(A).__name__})")
    G, P = input_ids.shape
    if torch.is_tensor(constraints) and constraints.dim() != 1:
        raise ValueError(f"generate(automaton=...) takes positional constraints of shape ({N},), one row for the batch: per-row masks "
                         f"{tuple(constraints.shape)} together with an automaton are out of scope")
    if A.V != V:
        raise ValueError(f"the automaton reads {A.V} tokens (the columns of delta) and the logits have {V} columns")
    Vlive = V if vocab_size is None else int(vocab_size)
    allow, check_masks = _allowed_masks(allowed_tokens, constraints, min_new_tokens, eos_token_id, G, fan, N, dev)
    check_masks(V, Vlive)
    # nothing depends on the position where the masks are one set for every token (allowed_tokens alone) and eos is not held back
    positional = constraints is not None or bool(int(min_new_tokens)) or not bool(A.accept.all())
    M = automaton_step_tables(A, N, masks=allow, eos=eos_token_id, vocab=Vlive, positional=positional)
    ctx = min(A.context, P)
    if ctx == 0:
        tails = [[] for _ in range(G)]
    elif lengths is None:
        tails = input_ids[:, P - ctx:].tolist()
    else:                                              # the tokens in front of lengths[b]
        idx = lengths.to(torch.int64)[:, None] - ctx + torch.arange(ctx, device=dev)
        got = torch.stack([input_ids.gather(1, idx.clamp(min=0)), idx]).tolist()
        tails = [[v for v, j in zip(row, at) if j >= 0] for row, at in zip(*got)]
    s0 = [A.initial_state(t) for t in tails]
    live0 = M[0] != 0
    for g, st in enumerate(s0):
        if not bool(live0[st]):
            raise ValueError(f"row {g}: after its prompt the automaton stands in state {st}, from which no accepted word of {N} new tokens "
                             "exists under these constraints")
    dstate = torch.tensor(s0, dtype=torch.int32).repeat_interleave(fan).to(dev)
    return M.to(dev), A.delta.to(dev), dstate


class GenerationMixin:
    """Greedy / top-k sampling.  Default: by re-running the causal model on the growing prefix (the reference's way: its HyenaOperator
    ignores ``inference_params``).  ``use_cache=True``: one prefill that fills every layer's decode cache, then one incremental step per
    token (hyena_dna_amd/inference.py); ``cg=True`` in addition replays the whole per-token step as one captured hipGraph
    (``GraphedDecodeStep``).  Sampling is the same code either way."""

    def allocate_inference_cache(self, batch_size, max_seqlen, dtype=None, **kwargs):
        return None

    @torch.no_grad()
    def generate(self, input_ids, max_length, top_k=1, temperature=1.0, return_dict_in_generate=False, output_scores=False, use_cache=False,
                 cg=False, lengths=None, pad_token_id=None, top_p=1.0, eos_token_id=None, seed=None, vocab_size=None, sampler=None,
                 stop_check_every=0, num_return_sequences=1, lookahead=None, allowed_tokens=None, constraints=None, min_new_tokens=0,
                 output_logprobs=False, num_beams=None, automaton=None, **kwargs):
        """``lengths`` (device int32 (B,), 1 <= lengths[b] <= P): ``input_ids`` (B, P) is right-padded and row b's prompt is its first
        lengths[b] tokens.  Every row then gets N = max_length - P new tokens, row b's i-th at column lengths[b] + i of the returned
        (B, max_length) ``sequences``; the columns from lengths[b] + N on hold ``pad_token_id`` (default: the model's ``pad_token_id``
        attribute where it has one, else 0).  Needs ``use_cache=True`` (each layer's cache keeps one position per row).

        ``sampler``: ``"torch"`` -- torch ops between the steps (top-k, torch's global generator) -- or ``"device"``: one HIP kernel at the
        end of every step (``inference.DeviceSampler``; with ``cg=True`` the last node of the replayed graph) that also serves ``top_p``
        (nucleus sampling), ``eos_token_id`` (a row that emits it is finished: ``pad_token_id`` from there on, the other rows continue),
        ``seed`` (the draws are a pure function of (seed, row, column); None: one seed from torch's generator per call) and ``vocab_size``
        (logit columns from there on, the padded vocabulary, are never chosen).  None: ``"device"`` when any of those four is given, else
        ``"torch"``.  ``stop_check_every=K > 0`` reads on the host every K tokens whether every row has finished and stops early (0: the
        loop never reads anything back).  The device sampler is a total function of its logits (it ends a captured graph and cannot raise):
        a NaN ranks before every number, the first NaN first (``torch.argmax``, ``torch.sort(descending=True, stable=True)``), and a row
        whose top-ranked logit is NaN or infinite emits that token whatever ``top_k``, ``top_p`` and ``temperature`` are -- always an id
        below ``vocab_size``; ``scores`` keep the NaN for the caller to see.

        ``num_return_sequences=n > 1``: n continuations of every prompt.  ``input_ids`` (G, P) -> ``sequences`` (G n, max_length), row
        g n + j being sample j of prompt g; ``scores`` are those of a batch of G n rows.  Needs ``use_cache=True``: the prefill runs once
        over the G prompts, every row's first token is drawn from its prompt's last logits, and each layer's cache keeps the history below
        ``(P // 8192) * 8192`` once per prompt (``HyenaDecodeState`` with ``fan=n``), so neither the prefill, nor the cache, nor the bytes
        a step streams below that point grow with n.  The step's results are those of ``generate(input_ids.repeat_interleave(n, 0))`` bit
        for bit.  Under the device sampler the rows of a group differ because the draw depends on the row index (under ``"torch"``
        through the global generator); greedy rows are all equal.  A prompt shorter than 8192 positions shares nothing in the step, which
        is launch-bound there -- it still saves the prefill.  Not together with ``lengths``.

        ``lookahead=W`` (1 ... 64; None / 0: off, today's step launch for launch): every layer's cache takes the history's share of the
        next W outputs ahead, one pass over the history per W tokens, and a step reads that carry and the columns written since, not the
        whole prompt (``HyenaDecodeState``).  The same sums in another order: logits differ from the plain cached step's by fp32 rounding.
        Needs ``use_cache=True``; works with both samplers, ``stop_check_every`` and ``cg=True`` (one replay per token, plus one group of
        refresh launches every W tokens).  Not with ``lengths`` or ``num_return_sequences > 1`` (out of scope, follow-ups).

        Which tokens may come out, and how likely they were (device sampler only; each selects it when ``sampler`` is None).
        ``allowed_tokens``: a sequence of ids, the only ones any new position may take.  ``constraints``: int64 bit masks on the input's
        device, (N,) or (B, N) with N = max_length - P -- bit v of constraints[b, i] lets token v be row b's i-th new token, also for
        ragged prompts (``inference.token_mask``, ``inference.iupac_constraints``); with ``num_return_sequences=n`` a (G, N) tensor holds
        one row per prompt.  Both given: the intersection.  ``min_new_tokens=m`` takes ``eos_token_id`` out of the first m positions.
        Ranks, top-k, the nucleus and greedy are taken among the allowed tokens only.  The masks are checked once on entry (one
        read-back): a position that allows no token below ``vocab_size`` is a ValueError.  ``output_logprobs=True`` adds ``logprobs``
        (B, number of steps run) fp32 to the returned tuple: the log-probability of every emitted token under the softmax of its live
        logits at temperature 1 -- the model's own distribution, not the constrained or tempered one -- NaN where the logits hold a NaN
        or +inf and for the positions of a finished row.

        ``num_beams=k`` (2 ... 16; None / 1: everything above, launch for launch): beam search -- the k most likely continuations found by
        keeping the k best prefixes per prompt at every step, scored by the sum of their tokens' log-probabilities under the model
        (temperature 1, all live tokens: the ``logprobs`` above).  ``input_ids`` (G, P); the cache is a fan-out cache with ``fan=k``, the
        beams of prompt g being its rows g k ... g k + k - 1: one prefill over the G prompts, then per token one step that ends with
        the beam kernel and one re-parenting of every layer's cache (``inference.BeamSearcher``, ``HyenaDecodeState.reorder``), which moves
        the columns written since the prompt only.  With ``cg=True`` the N - 1 steps are N - 1 replays of one graph.  Returned: the
        ``num_return_sequences = n <= k`` best beams per prompt, best first, row g n + r being rank r of prompt g; the tuple carries
        ``sequences`` (G n, max_length), ``scores=None``, ``sequences_scores`` (G n,) fp32 and, with ``output_logprobs=True``,
        ``logprobs`` (G n, steps run), whose rows sum to the scores.  Served with beams: ``allowed_tokens``, ``constraints`` ((N,) or
        (G, N)), ``min_new_tokens``, ``eos_token_id`` (a finished beam keeps its score, holds ``pad_token_id`` from there on and competes
        as it is), ``pad_token_id``, ``vocab_size``, ``stop_check_every``, ``cg``.  A beam that no allowed token can continue with a
        finite probability has score -inf.  Refused: ``use_cache=False``, ``sampler="torch"``, ``top_k > 1``, ``top_p != 1``,
        ``temperature != 1``, ``seed``, ``output_scores``, ``lengths``, ``lookahead``, n > k, logits of more than 64 columns.  Out of
        scope: a length penalty or any length normalisation, diverse or sampled beams, beams on ragged or lookahead caches.

        ``automaton=A`` (``inference.TokenAutomaton``, ``inference.motif_automaton``; device sampler and beams only, selects the device
        sampler when ``sampler`` is None): every returned row, up to its eos or to N new tokens, spells a word the automaton accepts --
        no restriction site on either strand, no homopolymer longer than h, a required motif somewhere, any regular language of at most
        4096 states over the logit columns.  The allowed set of a row depends on what the row has emitted: its state lives in device
        memory next to ``col`` and the sampler (the beam kernel) looks the mask up in a table computed backwards from the end on entry, so
        a row can never paint itself into a corner and a constrained generation is still N - 1 replays with ``cg=True``.  The last
        ``A.context`` prompt tokens set the initial state.  Composes with everything above: ``allowed_tokens``, ``constraints`` ((N,)
        only), ``min_new_tokens``, ``eos_token_id`` (allowed only in an accepting state), ``vocab_size``, ``top_k``, ``top_p``,
        ``temperature``, ``seed``, ``lengths``, ``num_return_sequences``, ``lookahead``, ``stop_check_every``, ``output_scores``,
        ``output_logprobs``, ``num_beams``, ``cg``.  ValueError: ``sampler="torch"``, ``use_cache=False``, (B, N) constraints, an
        automaton whose ``delta`` has another number of columns than the logits, a prompt after which no accepted word of N tokens
        exists (the row is named), N S over 2^22 where the table depends on the position."""
        if num_beams is not None and int(num_beams) != 1:
            return self._generate_beam(input_ids, max_length, int(num_beams), int(num_return_sequences), top_k=top_k, temperature=temperature,
                                       return_dict_in_generate=return_dict_in_generate, output_scores=output_scores, use_cache=use_cache,
                                       cg=cg, lengths=lengths, pad_token_id=pad_token_id, top_p=top_p, eos_token_id=eos_token_id, seed=seed,
                                       vocab_size=vocab_size, sampler=sampler, stop_check_every=int(stop_check_every), lookahead=lookahead,
                                       allowed_tokens=allowed_tokens, constraints=constraints, min_new_tokens=min_new_tokens,
                                       output_logprobs=output_logprobs, automaton=automaton)
        if cg and not use_cache:
            raise ValueError("generate(cg=True) replays the cached step: it needs use_cache=True")
        from .inference import check_lookahead
        W = check_lookahead(lookahead)
        if W and not use_cache:
            raise ValueError("generate(lookahead=W) carries the history's share of the cached step: it needs use_cache=True")
        if W and lengths is not None:
            raise NotImplementedError("generate(lookahead=W, lengths=...): lookahead for ragged prompts is out of scope (one position per batch)")
        if W and int(num_return_sequences) > 1:
            raise NotImplementedError("generate(lookahead=W, num_return_sequences > 1): lookahead for fan-out caches is out of scope")
        n = int(num_return_sequences)
        if n < 1:
            raise ValueError(f"num_return_sequences={num_return_sequences}: at least one continuation per prompt")
        if n > 1 and not use_cache:
            raise ValueError("generate(num_return_sequences > 1) shares the prompt through the decode cache: it needs use_cache=True")
        if n > 1 and lengths is not None:
            raise NotImplementedError("generate(num_return_sequences > 1, lengths=...): ragged prompts with fan-out are out of scope "
                                      "(the shared history needs one prompt length)")
        wants_device = [n for n, on in (("top_p", top_p is not None and float(top_p) != 1.0), ("eos_token_id", eos_token_id is not None),
                                        ("seed", seed is not None), ("vocab_size", vocab_size is not None),
                                        ("allowed_tokens", allowed_tokens is not None), ("constraints", constraints is not None),
                                        ("min_new_tokens", bool(min_new_tokens)), ("output_logprobs", bool(output_logprobs)),
                                        ("automaton", automaton is not None)) if on]
        if sampler is None:
            sampler = "device" if wants_device else "torch"
        if sampler not in ("torch", "device"):
            raise ValueError(f"sampler={sampler!r}: 'torch', 'device' or None")
        if sampler == "device":
            return self._generate_device(input_ids, max_length, lengths, pad_token_id, top_k, temperature, return_dict_in_generate, output_scores,
                                         use_cache, cg, 1.0 if top_p is None else float(top_p), eos_token_id, seed, vocab_size,
                                         int(stop_check_every), fan=n, lookahead=W, allowed_tokens=allowed_tokens, constraints=constraints,
                                         min_new_tokens=min_new_tokens, output_logprobs=output_logprobs, automaton=automaton)
        if wants_device or stop_check_every:
            raise ValueError(f"sampler='torch' does not serve {', '.join(wants_device + ['stop_check_every'] * bool(stop_check_every))}: "
                             "use sampler='device'")
        if lengths is not None:
            return self._generate_ragged(input_ids, max_length, lengths, pad_token_id, top_k, temperature, return_dict_in_generate,
                                         output_scores, use_cache, cg)
        ids, scores = input_ids, []
        if not use_cache:
            while ids.shape[1] < max_length:
                logits, nxt = _sample(_last_logits(self(ids)), top_k, temperature)
                scores.append(logits)
                ids = torch.cat([ids, nxt], dim=1)
        elif ids.shape[1] < max_length:
            from .inference import InferenceParams
            B = ids.shape[0] * n
            ip = InferenceParams(max_seqlen=max_length, max_batch_size=B, lookahead=W)
            ip.key_value_memory_dict = self.allocate_inference_cache(B, max_length, **({} if n == 1 else dict(fan=n, prompt_len=ids.shape[1])),
                                                                     **(dict(lookahead=W) if W else {}))
            if ip.key_value_memory_dict is None:
                raise NotImplementedError(f"{type(self).__name__} has no decode cache: generate(use_cache=True) is not available")
            last = _last_logits(self(ids, inference_params=ip))
            if n > 1:                                  # one prefill over the G prompts; from here on G n rows
                last, ids = last.repeat_interleave(n, 0), ids.repeat_interleave(n, 0)
            ip.seqlen_offset = ids.shape[1]
            step = GraphedDecodeStep(self, ip, B) if cg else None
            try:
                while True:
                    logits, nxt = _sample(last, top_k, temperature)
                    scores.append(logits)
                    ids = torch.cat([ids, nxt], dim=1)
                    if ids.shape[1] >= max_length:
                        break
                    last = step(nxt) if cg else _last_logits(self(nxt, inference_params=ip))
                    ip.seqlen_offset += 1
            finally:
                if step is not None:
                    step.release()
        elif n > 1:                                    # nothing to generate: the rows of a group are the prompt
            ids = ids.repeat_interleave(n, 0)
        if return_dict_in_generate:
            return namedtuple("GreedySearchDecoderOnlyOutput", ["sequences", "scores"])(ids, tuple(scores) if output_scores else None)
        return ids


    def _generate_device(self, input_ids, max_length, lengths, pad_token_id, top_k, temperature, return_dict_in_generate, output_scores,
                         use_cache, cg, top_p, eos_token_id, seed, vocab_size, stop_check_every, fan=1, lookahead=0, allowed_tokens=None,
                         constraints=None, min_new_tokens=0, output_logprobs=False, automaton=None):
        """generate() with the device sampler: the prefill, one eager sampler call on its last logits (row b's own last position for ragged
        prompts), then N - 1 steps that each end with the sampler kernel writing the next step's input ids in place -- with ``cg`` N - 1
        graph replays and no tensor work between them.  ``sequences`` is one (B, max_length) tensor allocated up front.  ``fan = n > 1``:
        ``input_ids`` holds G prompts, B = G n rows; the prefill runs over the prompts and row g n + j draws from prompt g's last logits."""
        from . import _lib
        from .inference import DeviceSampler, InferenceParams
        if not use_cache:
            raise ValueError("generate(sampler='device') samples at the end of the cached step: it needs use_cache=True")
        if not 0.0 < top_p <= 1.0:
            raise ValueError(f"top_p={top_p}: the nucleus mass lies in (0, 1]")
        if stop_check_every < 0:
            raise ValueError(f"stop_check_every={stop_check_every}: a number of tokens, or 0 for never")
        dev = input_ids.device
        if not (dev.type == "cuda" or _lib._backend.name != "hip"):
            raise NotImplementedError(f"generate(sampler='device') runs a HIP kernel: the model and input_ids must live on a ROCm device (got {dev})")
        B, P = input_ids.shape
        B *= fan
        ragged = lengths is not None
        if ragged:
            if not torch.is_tensor(lengths) or lengths.shape != (B,) or lengths.dtype != torch.int32 or lengths.device != dev:
                what = f"{tuple(lengths.shape)} {lengths.dtype} on {lengths.device}" if torch.is_tensor(lengths) else type(lengths).__name__
                raise ValueError(f"lengths must be a ({B},) int32 tensor on {dev} (got {what})")
            lo, hi = (int(v) for v in torch.stack([lengths.min(), lengths.max()]).tolist())        # the one host read
            if lo < 1 or hi > P:
                raise ValueError(f"lengths must lie in [1, {P}] (the padded prompt has {P} columns; got {lo} ... {hi})")
            emb = getattr(getattr(self, "backbone", None), "embeddings", None)
            if getattr(emb, "max_position_embeddings", 0) > 0:
                raise NotImplementedError("generate(lengths=...) with learned position embeddings (one position id per row) is not implemented")
        if pad_token_id is None:
            pad_token_id = getattr(self, "pad_token_id", None)
        pad_token_id = 0 if pad_token_id is None else int(pad_token_id)
        N = max(int(max_length) - P, 0)
        seq = torch.full((B, P + N), pad_token_id, dtype=torch.int64, device=dev)
        if ragged:
            cols = torch.arange(P, device=dev)
            seq[:, :P] = torch.where(cols[None] < lengths[:, None], input_ids, seq[:, :P])
            col = lengths.clone()
        else:
            seq[:, :P] = input_ids if fan == 1 else input_ids.repeat_interleave(fan, 0)
            col = torch.full((B,), P, dtype=torch.int32, device=dev)
        smp, n_done = None, 0
        tables = None
        if automaton is not None and N > 0:            # every refusal before a cache exists; V from the head (checked against the logits below)
            head = getattr(self, "lm_head", None)
            V_head = head.weight.shape[0] if torch.is_tensor(getattr(head, "weight", None)) else automaton.V
            if vocab_size is not None and not 1 <= int(vocab_size) <= V_head:
                raise ValueError(f"vocab_size={vocab_size}: the logits have {V_head} columns")
            tables = _automaton_tables(automaton, input_ids, lengths, fan, N, V_head, vocab_size, allowed_tokens, constraints, min_new_tokens,
                                       eos_token_id)
        if N > 0:
            ip = InferenceParams(max_seqlen=P + N, max_batch_size=B, lengths_per_sample=lengths, lookahead=lookahead)
            ip.key_value_memory_dict = self.allocate_inference_cache(B, P + N, **({} if fan == 1 else dict(fan=fan, prompt_len=P)),
                                                                     **(dict(lookahead=lookahead) if lookahead else {}))
            if ip.key_value_memory_dict is None:
                raise NotImplementedError(f"{type(self).__name__} has no decode cache: generate(use_cache=True) is not available")
            if tables is None:
                allow, check_masks = _allowed_masks(allowed_tokens, constraints, min_new_tokens, eos_token_id, B // fan, fan, N, dev)
            else:                                      # (the positional masks are inside M)
                allow, check_masks = None, lambda V, Vlive: None
            out = self(input_ids, inference_params=ip)
            logits = out[0] if isinstance(out, tuple) else out
            logits = logits.logits if hasattr(logits, "logits") else logits                        # (B, P, V); fan > 1: (B / fan, P, V)
            V = logits.shape[-1]
            if V > _lib.SAMPLE_MAX_V:
                raise ValueError(f"generate(sampler='device') serves logits of at most {_lib.SAMPLE_MAX_V} columns (this model has {V})")
            if vocab_size is not None and not 1 <= int(vocab_size) <= V:
                raise ValueError(f"vocab_size={vocab_size}: the logits have {V} columns")
            if ragged:
                last = logits.gather(1, (lengths.to(torch.int64) - 1)[:, None, None].expand(B, 1, V))[:, 0]
            else:
                last = logits[:, -1] if fan == 1 else logits[:, -1].repeat_interleave(fan, 0)
            if seed is None:                           # torch's generator, once per call (greedy draws nothing)
                seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item()) if top_k > 1 else 0
            seed = torch.tensor([int(seed)], dtype=torch.int64).to(dev)
            check_masks(V, V if vocab_size is None else int(vocab_size))
            if tables is not None and tables[1].shape[1] != V:
                raise ValueError(f"the automaton reads {tables[1].shape[1]} tokens (the columns of delta) and the logits have {V} columns")
            smp = DeviceSampler(seq, col, seed, temperature=temperature, top_k=top_k, top_p=top_p, eos=eos_token_id, pad=pad_token_id,
                                vocab=vocab_size, want_scores=output_scores, V=V, allow=allow, want_logprobs=output_logprobs, n_new=N,
                                **({} if tables is None else dict(automaton_tables=tables)))
            ip.seqlen_offset = P                       # ragged: the furthest any row has got (bounds checks only)
            step = GraphedDecodeStep(self, ip, B, sampler=smp) if cg and N > 1 else None
            nxt = step.ids if step is not None else torch.empty(B, 1, dtype=torch.int64, device=dev)
            try:
                smp(last, nxt)
                n_done = 1
                for i in range(1, N):
                    if stop_check_every and i % stop_check_every == 0 and bool(smp.done.all()):
                        break
                    if step is not None:
                        step.replay()
                    else:
                        smp(_last_logits(self(nxt, inference_params=ip)), nxt)
                    ip.seqlen_offset += 1
                    n_done = i + 1
            finally:
                if step is not None:
                    step.release()
        if not return_dict_in_generate:
            return seq
        scores = None
        if output_scores:
            if smp is None:
                scores = ()
            elif ragged:                               # row b's i-th new token stands at column lengths[b] + i
                idx = (lengths.to(torch.int64)[:, None] + torch.arange(n_done, device=dev))[:, :, None].expand(B, n_done, smp.scores.shape[2])
                scores = tuple(smp.scores.gather(1, idx).unbind(1))
            else:
                scores = tuple(smp.scores[:, P:P + n_done].contiguous().unbind(1))
        fields, values = ["sequences", "scores"], [seq, scores]
        if ragged:
            fields, values = fields + ["lengths"], values + [lengths + N]
        if output_logprobs:                            # row b's i-th new token at [b, i], ragged or not
            fields.append("logprobs")
            values.append(torch.empty(B, 0, device=dev) if smp is None else smp.logprobs[:, :n_done].contiguous())
        return namedtuple("GreedySearchDecoderOnlyOutput", fields)(*values)


    def _generate_beam(self, input_ids, max_length, k, n, top_k=1, temperature=1.0, return_dict_in_generate=False, output_scores=False,
                       use_cache=False, cg=False, lengths=None, pad_token_id=None, top_p=1.0, eos_token_id=None, seed=None, vocab_size=None,
                       sampler=None, stop_check_every=0, lookahead=None, allowed_tokens=None, constraints=None, min_new_tokens=0,
                       output_logprobs=False, automaton=None):
        """generate(num_beams=k): the prefill over the G prompts into a fan-out cache (fan = k), one eager beam step on its last logits,
        then N - 1 steps that each end with the beam kernel and the caches' re-parenting (``inference.BeamSearcher``) -- with ``cg`` N - 1
        graph replays -- and one backtrack over the records.  Every refusal comes before a cache is built."""
        from . import _lib
        from .inference import BeamSearcher, InferenceParams, check_lookahead
        if not 2 <= k <= _lib.DECODE_BEAM_MAX:
            raise ValueError(f"num_beams={k}: 2 ... {_lib.DECODE_BEAM_MAX} beams per prompt (None or 1: no beam search)")
        if not use_cache:
            raise ValueError("generate(num_beams=k) keeps the beams in a fan-out decode cache: it needs use_cache=True")
        if sampler not in (None, "device"):
            raise ValueError(f"generate(num_beams=k) with sampler={sampler!r}: the beam step is a device kernel (sampler='device' or None)")
        if not 1 <= n <= k:
            raise ValueError(f"num_return_sequences={n}: 1 ... num_beams = {k} of the beams can be returned")
        nothing = [name for name, on in (("top_k > 1", int(top_k) > 1), ("top_p != 1", top_p is not None and float(top_p) != 1.0),
                                         ("temperature != 1", float(temperature) != 1.0), ("seed", seed is not None),
                                         ("output_scores", bool(output_scores))) if on]
        if nothing:
            raise ValueError(f"generate(num_beams=k) is a deterministic search on the model's own log-probabilities: it does not serve "
                             f"{', '.join(nothing)}")
        if lengths is not None:
            raise NotImplementedError("generate(num_beams=k, lengths=...): beams on ragged caches are out of scope")
        if check_lookahead(lookahead):
            raise NotImplementedError("generate(num_beams=k, lookahead=W): beams on lookahead caches are out of scope")
        if stop_check_every < 0:
            raise ValueError(f"stop_check_every={stop_check_every}: a number of tokens, or 0 for never")
        head = getattr(self, "lm_head", None)
        V = head.weight.shape[0] if torch.is_tensor(getattr(head, "weight", None)) else None
        if V is not None and V > _lib.SAMPLE_MAX_V:
            raise ValueError(f"generate(num_beams=k) serves logits of at most {_lib.SAMPLE_MAX_V} columns (this model has {V})")
        if vocab_size is not None and V is not None and not 1 <= int(vocab_size) <= V:
            raise ValueError(f"vocab_size={vocab_size}: the logits have {V} columns")
        dev = input_ids.device
        if not (dev.type == "cuda" or _lib._backend.name != "hip"):
            raise NotImplementedError(f"generate(num_beams=k) runs HIP kernels: the model and input_ids must live on a ROCm device (got {dev})")
        G, P = input_ids.shape
        B = G * k
        if pad_token_id is None:
            pad_token_id = getattr(self, "pad_token_id", None)
        pad_token_id = 0 if pad_token_id is None else int(pad_token_id)
        N = max(int(max_length) - P, 0)
        fields = ["sequences", "scores", "sequences_scores"] + ["logprobs"] * bool(output_logprobs)
        if N == 0:                                     # nothing to generate: every beam is the prompt
            seq = input_ids.repeat_interleave(n, 0)
            if not return_dict_in_generate:
                return seq
            values = [seq, None, torch.zeros(G * n, dtype=torch.float32, device=dev)] + [torch.empty(G * n, 0, device=dev)] * bool(output_logprobs)
            return namedtuple("BeamSearchDecoderOnlyOutput", fields)(*values)
        tables = None
        if automaton is not None:                      # every refusal before a cache exists; the positional masks go into M
            tables = _automaton_tables(automaton, input_ids, None, k, N, automaton.V if V is None else V, vocab_size, allowed_tokens,
                                       constraints, min_new_tokens, eos_token_id)
            allow, check_masks = None, lambda V, Vlive: None
        else:
            allow, check_masks = _allowed_masks(allowed_tokens, constraints, min_new_tokens, eos_token_id, G, k, N, dev)
        if V is not None:
            check_masks(V, V if vocab_size is None else int(vocab_size))
        ip = InferenceParams(max_seqlen=P + N, max_batch_size=B)
        ip.key_value_memory_dict = self.allocate_inference_cache(B, P + N, fan=k, prompt_len=P)
        if ip.key_value_memory_dict is None:
            raise NotImplementedError(f"{type(self).__name__} has no decode cache: generate(use_cache=True) is not available")
        out = self(input_ids, inference_params=ip)
        logits = out[0] if isinstance(out, tuple) else out
        logits = logits.logits if hasattr(logits, "logits") else logits                            # (G, P, V)
        if V is None:
            V = logits.shape[-1]
            if V > _lib.SAMPLE_MAX_V:
                raise ValueError(f"generate(num_beams=k) serves logits of at most {_lib.SAMPLE_MAX_V} columns (this model has {V})")
            if vocab_size is not None and not 1 <= int(vocab_size) <= V:
                raise ValueError(f"vocab_size={vocab_size}: the logits have {V} columns")
            check_masks(V, V if vocab_size is None else int(vocab_size))
        if tables is not None and tables[1].shape[1] != logits.shape[-1]:
            raise ValueError(f"the automaton reads {tables[1].shape[1]} tokens (the columns of delta) and the logits have {logits.shape[-1]} columns")
        last = logits[:, -1].repeat_interleave(k, 0)
        search = BeamSearcher(ip.key_value_memory_dict.values(), input_ids, k, N, eos=eos_token_id, pad=pad_token_id, vocab=vocab_size, allow=allow,
                              **({} if tables is None else dict(automaton_tables=tables)))
        ip.seqlen_offset = P
        step = GraphedDecodeStep(self, ip, B, sampler=search) if cg and N > 1 else None
        nxt = step.ids if step is not None else torch.empty(B, 1, dtype=torch.int64, device=dev)
        try:
            search(last, nxt)
            n_done = 1
            for i in range(1, N):
                if stop_check_every and i % stop_check_every == 0 and bool(search.done.all()):
                    break
                if step is not None:
                    step.replay()
                else:
                    search(_last_logits(self(nxt, inference_params=ip)), nxt)
                ip.seqlen_offset += 1
                n_done = i + 1
        finally:
            if step is not None:
                step.release()
        seq, scores, logprobs = search.finalize(n_done, n, want_logprobs=output_logprobs)
        if not return_dict_in_generate:
            return seq
        return namedtuple("BeamSearchDecoderOnlyOutput", fields)(*([seq, None, scores] + [logprobs] * bool(output_logprobs)))


    def _generate_ragged(self, input_ids, max_length, lengths, pad_token_id, top_k, temperature, return_dict_in_generate, output_scores,
                         use_cache, cg):
        """generate() over right-padded prompts of different lengths: one prefill over the padded batch (causal model: the positions below
        lengths[b] are those of the unpadded prompt), the first token of row b from the logits at position lengths[b] - 1, then per-row
        decode steps.  One host check of ``lengths`` on entry; nothing in the loop reads them on the host."""
        from .inference import InferenceParams
        if not use_cache:
            raise ValueError("generate(lengths=...) decodes every row at its own position, which only the cached step does: it needs use_cache=True")
        B, P = input_ids.shape
        if not torch.is_tensor(lengths) or lengths.shape != (B,) or lengths.dtype != torch.int32 or lengths.device != input_ids.device:
            what = f"{tuple(lengths.shape)} {lengths.dtype} on {lengths.device}" if torch.is_tensor(lengths) else type(lengths).__name__
            raise ValueError(f"lengths must be a ({B},) int32 tensor on {input_ids.device} (got {what})")
        lo, hi = (int(v) for v in torch.stack([lengths.min(), lengths.max()]).tolist())            # the one host read
        if lo < 1 or hi > P:
            raise ValueError(f"lengths must lie in [1, {P}] (the padded prompt has {P} columns; got {lo} ... {hi})")
        emb = getattr(getattr(self, "backbone", None), "embeddings", None)
        if getattr(emb, "max_position_embeddings", 0) > 0:
            raise NotImplementedError("generate(lengths=...) with learned position embeddings (one position id per row) is not implemented")
        if pad_token_id is None:
            pad_token_id = getattr(self, "pad_token_id", None)
        pad_token_id = 0 if pad_token_id is None else int(pad_token_id)
        N = max(int(max_length) - P, 0)
        len64 = lengths.to(torch.int64)
        cols = torch.arange(P + N, device=input_ids.device)
        seq = torch.full((B, P + N), pad_token_id, dtype=input_ids.dtype, device=input_ids.device)
        seq[:, :P] = torch.where(cols[None, :P] < len64[:, None], input_ids, seq[:, :P])
        scores = []
        if N > 0:
            ip = InferenceParams(max_seqlen=P + N, max_batch_size=B, lengths_per_sample=lengths)
            ip.key_value_memory_dict = self.allocate_inference_cache(B, P + N)
            if ip.key_value_memory_dict is None:
                raise NotImplementedError(f"{type(self).__name__} has no decode cache: generate(use_cache=True) is not available")
            out = self(input_ids, inference_params=ip)
            logits = out[0] if isinstance(out, tuple) else out
            logits = logits.logits if hasattr(logits, "logits") else logits                        # (B, P, V): row b's last prompt position
            last = logits.gather(1, (len64 - 1)[:, None, None].expand(B, 1, logits.shape[-1]))[:, 0]
            ip.seqlen_offset = P                       # the furthest any row has got: bounds checks only, the kernels read the per-row positions
            step = GraphedDecodeStep(self, ip, B) if cg else None
            try:
                for i in range(N):
                    logits, nxt = _sample(last, top_k, temperature)
                    scores.append(logits)
                    seq.scatter_(1, (len64 + i)[:, None], nxt)
                    if i == N - 1:
                        break
                    last = step(nxt) if cg else _last_logits(self(nxt, inference_params=ip))
                    ip.seqlen_offset += 1
            finally:
                if step is not None:
                    step.release()
        if return_dict_in_generate:
            return namedtuple("GreedySearchDecoderOnlyOutput", ["sequences", "scores", "lengths"])(
                seq, tuple(scores) if output_scores else None, lengths + N)
        return seq


def sync_shared_params(model, process_group):
    """Broadcast parameters marked ``_shared_params`` from rank 0 of the group (flash_attn.utils.distributed)."""
    import torch.distributed as dist
    for _, p in sorted(model.named_parameters()):
        if getattr(p, "_shared_params", False):
            with torch.no_grad():
                dist.broadcast(p, src=dist.get_global_rank(process_group, 0), group=process_group)


def all_gather_raw(input_, process_group, async_op=False):
    import torch.distributed as dist
    world = dist.get_world_size(process_group)
    out = torch.empty(world * input_.shape[0], *input_.shape[1:], dtype=input_.dtype, device=input_.device)
    handle = dist.all_gather_into_tensor(out, input_.contiguous(), group=process_group, async_op=async_op)
    return out, handle


# ---------------------------------------------------------------------------------------------------------------------
# The hyenadna-* language model without Lightning / Hydra (structure: long_conv_lm.py:249-502, hg38_hyena.yaml)
# ---------------------------------------------------------------------------------------------------------------------
def _init_weights(module, n_layer, initializer_range=0.02, rescale_prenorm_residual=True):
    """long_conv_lm.py:204-246 (GPT-2 scheme: out_proj / fc2 scaled by 1 / sqrt(2 n_layer))."""
    if isinstance(module, nn.Linear):
        nn.init.normal_(module.weight, std=initializer_range)
        if module.bias is not None:
            nn.init.zeros_(module.bias)
    elif isinstance(module, nn.Embedding):
        nn.init.normal_(module.weight, std=initializer_range)
    if rescale_prenorm_residual:
        for name, p in module.named_parameters():
            if name in ("out_proj.weight", "fc2.weight"):
                nn.init.normal_(p, mean=0.0, std=initializer_range / math.sqrt(2 * n_layer))


class HyenaDNALM(nn.Module, GenerationMixin):
    """``ConvLMHeadModel`` with the Hyena mixer in every block (the hg38 pre-training model): same sub-module names as the
    reference (``backbone.embeddings.word_embeddings``, ``backbone.layers.N.{mixer,norm1,norm2,mlp.fc1,mlp.fc2}``,
    ``backbone.ln_f``, ``lm_head``), so a reference checkpoint's state dict loads."""

    def __init__(self, d_model, n_layer, d_inner, vocab_size, layer=None, max_position_embeddings=0, resid_dropout=0.0,
                 embed_dropout=0.1, layer_norm_epsilon=1e-5, initializer_cfg=None, fused_dropout_add_ln=True,
                 residual_in_fp32=True, pad_vocab_size_multiple=1, checkpoint_mixer=False, checkpoint_mlp=False, **unused):
        super().__init__()
        from .hyena import HyenaOperator
        # Keywords of ConvLMHeadModel / LMBackbone (long_conv_lm.py:249-272, 402-424) this single-process, Hyena-only model has
        # no counterpart for are accepted at their "off" values only: a config asking for attention layers, tensor parallelism
        # or flash_attn's FusedMLP must not silently get a different model.
        off = {"attn_layer_idx": None, "attn_cfg": None, "process_group": None, "fused_mlp": False, "identity_mlp": False,
               "sequence_parallel": (True, False), "return_hidden_state": False}
        # the factory keywords every reference module takes (long_conv_lm.py:266: factory_kwargs): applied after construction
        device, dtype = unused.pop("device", None), unused.pop("dtype", None)
        for key, val in unused.items():
            allowed = off.get(key, KeyError)
            if allowed is KeyError:
                raise TypeError(f"HyenaDNALM: unknown keyword {key!r}")
            if not (val in allowed if isinstance(allowed, tuple) else val == allowed):
                raise NotImplementedError(f"HyenaDNALM: {key}={val!r} is not supported (Hyena mixers, one process per GPU, "
                                          "library-GEMM MLP only)")
        if vocab_size % pad_vocab_size_multiple != 0:
            vocab_size += pad_vocab_size_multiple - (vocab_size % pad_vocab_size_multiple)
        layer = dict(layer or {})
        layer.pop("_name_", None)
        self.d_model, self.residual_in_fp32, self.fused_dropout_add_ln = d_model, residual_in_fp32, fused_dropout_add_ln
        backbone = nn.Module()
        backbone.embeddings = GPT2Embeddings(d_model, vocab_size, max_position_embeddings)
        mlp_cls = partial(Mlp, hidden_features=d_inner if d_inner is not None else 4 * d_model,
                          activation=partial(F.gelu, approximate="tanh"))
        norm_cls = partial(nn.LayerNorm, eps=layer_norm_epsilon)
        backbone.layers = nn.ModuleList([
            Block(d_model, partial(HyenaOperator, **layer), mlp_cls, norm_cls=norm_cls, prenorm=True,
                  resid_dropout1=embed_dropout if i == 0 else resid_dropout, resid_dropout2=resid_dropout,
                  fused_dropout_add_ln=fused_dropout_add_ln, residual_in_fp32=residual_in_fp32) for i in range(n_layer)])
        # long_conv_lm.py:196-199: activation checkpointing wraps the sub-module, which also moves its state-dict keys under
        # `.layer` -- a checkpoint saved with these flags loads only into a model built with them
        for blk in backbone.layers:
            if checkpoint_mlp:
                blk.mlp = CheckpointedModule(blk.mlp)
            if checkpoint_mixer:
                blk.mixer = CheckpointedModule(blk.mixer)
        for i, blk in enumerate(backbone.layers):
            mixer = getattr(blk.mixer, "layer", blk.mixer)
            if isinstance(mixer, HyenaOperator) and mixer.layer_idx is None:
                mixer.layer_idx = i                       # the key of its decode cache (long_conv_lm.py:171-185 passes layer_idx the same way)
        backbone.drop_f = nn.Dropout(resid_dropout)
        backbone.ln_f = nn.LayerNorm(d_model, eps=layer_norm_epsilon)
        self.backbone = backbone
        self.checkpoint_mixer, self.checkpoint_mlp = checkpoint_mixer, checkpoint_mlp
        self.lm_head = nn.Linear(d_model, vocab_size, bias=False)
        self.apply(partial(_init_weights, n_layer=n_layer, **(initializer_cfg or {})))
        self.tie_weights()
        if device is not None or dtype is not None:
            self.to(device=device, dtype=dtype)

    def tie_weights(self):
        self.lm_head.weight = self.backbone.embeddings.word_embeddings.weight

    def hidden(self, input_ids, position_ids=None, inference_params=None, soft_tokens=None, soft_dropout_p=0.0):
        return self._final_norm(*self.trunk(input_ids, position_ids, inference_params=inference_params, soft_tokens=soft_tokens,
                                            soft_dropout_p=soft_dropout_p))

    def _embedding_fusion_ok(self, input_ids):
        """the first block's norm can gather the token embedding itself (block.embedding_fusable + this model's configuration)"""
        bb = self.backbone
        emb, blk0 = bb.embeddings, bb.layers[0]
        return (self.fused_dropout_add_ln and self.residual_in_fp32 and isinstance(blk0, Block) and blk0.prenorm and blk0.fused_dropout_add_ln
                and blk0.residual_in_fp32 and emb.project_in is None and emb.max_position_embeddings <= 0
                and embedding_fusable(input_ids, emb.word_embeddings, blk0.norm1.weight))

    def _trunk_soft(self, input_ids, position_ids, soft_tokens, soft_dropout_p, fused=True):
        """``trunk`` over ``[dropout(soft_tokens) | embeddings(input_ids)]`` (B, n + L, D): the reference's soft prompting
        (evals/soft_prompting_genomics.py LitModel.forward).  Token positions count from 0 and the soft tokens get no position embedding, as
        there.  Fused into the first block's norm (block.soft_embedding_dropout_add_layer_norm) when the embedding fusion applies, the kernels
        cover the shape and neither the table nor norm1 wants a gradient (the pass returns the soft tokens' gradient only); otherwise the
        reference's own statement, ``torch.cat``, in front of the blocks as they are."""
        from . import _lib
        bb = self.backbone
        emb, blk0 = bb.embeddings, bb.layers[0]
        if soft_tokens.dim() != 2 or soft_tokens.shape[1] != self.d_model or soft_tokens.shape[0] < 1:
            raise ValueError(f"soft_tokens has to be (n >= 1, {self.d_model}), got {tuple(soft_tokens.shape)}")
        B, L = input_ids.shape
        n = soft_tokens.shape[0]
        for mixer in self._mixers():
            l_max = getattr(mixer, "l_max", None)
            if l_max is not None and n + L > l_max:
                raise ValueError(f"{n} soft tokens + {L} positions = {n + L} exceed a mixer's l_max = {l_max}")
        sp = float(soft_dropout_p) if self.training else 0.0
        if (fused and self._embedding_fusion_ok(input_ids) and soft_tokens.dtype == torch.float32 and soft_tokens.device == input_ids.device
                and _lib.soft_embed_add_norm_supported(emb.word_embeddings.weight.shape[0], self.d_model, torch.float32)
                and not (torch.is_grad_enabled() and (emb.word_embeddings.weight.requires_grad or blk0.norm1.weight.requires_grad
                                                      or blk0.norm1.bias.requires_grad))):
            dev_type = input_ids.device.type
            odt = torch.get_autocast_dtype(dev_type) if torch.is_autocast_enabled(dev_type) else torch.float32
            if odt not in (torch.bfloat16, torch.float16):
                odt = torch.float32
            hidden_states, residual = soft_embedding_dropout_add_layer_norm(
                input_ids, emb.word_embeddings.weight, soft_tokens, blk0.norm1.weight, blk0.norm1.bias, blk0.dropout1.p if self.training else 0.0,
                sp, blk0.norm1.eps, out_dtype=odt)
            hidden_states, residual = blk0(hidden_states, residual, normed=True)
            rest = list(bb.layers)[1:]
        else:
            tokens = emb(input_ids, position_ids=position_ids)
            soft = F.dropout(soft_tokens, sp, training=True) if sp > 0.0 else soft_tokens
            hidden_states, residual = torch.cat([soft.to(tokens.dtype).unsqueeze(0).expand(B, n, self.d_model), tokens], 1), None
            rest = bb.layers
        for blk in rest:
            hidden_states, residual = blk(hidden_states, residual)
        return hidden_states, residual

    def trunk(self, input_ids, position_ids=None, inference_params=None, soft_tokens=None, soft_dropout_p=0.0, soft_fused=True):
        """(hidden_states, residual) as the last block leaves them, in front of drop_f / ln_f (long_conv_lm.py:367-380): what a readout that
        carries the final norm inside its own pass starts from (classifier.HyenaDNAClassifier).  ``soft_tokens`` (n, D): learnable embeddings in
        front of the tokens -- the outputs are (B, n + L, ...) (``_trunk_soft``); None: the token-only path."""
        if soft_tokens is not None:
            if inference_params is not None:
                raise NotImplementedError("cached decoding with a soft prefix is not supported")
            return self._trunk_soft(input_ids, position_ids, soft_tokens, soft_dropout_p, fused=soft_fused)
        bb = self.backbone
        emb, blk0 = bb.embeddings, bb.layers[0]
        # inference_params reach every mixer through the block's mixer_kwargs (long_conv_lm.py:375-378); a non-empty mixer_kwargs also keeps the
        # block off forward_add_norm
        mk = (lambda: None) if inference_params is None else (lambda: {"inference_params": inference_params})
        if self._embedding_fusion_ok(input_ids):
            # the token embedding gathered inside the first block's dropout -> add -> LayerNorm pass (block.py): neither the (B, L, D) fp32
            # embedding nor its gradient exists; the normed output leaves in the autocast type the mixer would round it to anyway
            dev_type = input_ids.device.type
            odt = torch.get_autocast_dtype(dev_type) if torch.is_autocast_enabled(dev_type) else torch.float32
            if odt not in (torch.bfloat16, torch.float16):
                odt = torch.float32
            hidden_states, residual = embedding_dropout_add_layer_norm(input_ids, emb.word_embeddings.weight, blk0.norm1.weight, blk0.norm1.bias,
                                                                       blk0.dropout1.p if self.training else 0.0, blk0.norm1.eps, out_dtype=odt)
            hidden_states, residual = blk0(hidden_states, residual, normed=True, mixer_kwargs=mk())
            rest = list(bb.layers)[1:]
        else:
            hidden_states, residual = emb(input_ids, position_ids=position_ids), None
            rest = bb.layers
        for blk in rest:
            hidden_states, residual = blk(hidden_states, residual, mixer_kwargs=mk())
        return hidden_states, residual

    def _final_norm(self, hidden_states, residual):
        """drop_f -> add -> ln_f (long_conv_lm.py:381-396)"""
        bb = self.backbone
        if self.fused_dropout_add_ln:
            return dropout_add_layer_norm(hidden_states, residual, bb.ln_f.weight, bb.ln_f.bias,
                                          bb.drop_f.p if self.training else 0.0, bb.ln_f.eps, prenorm=False,
                                          residual_in_fp32=self.residual_in_fp32)
        dropped = bb.drop_f(hidden_states)
        residual = (dropped + residual) if residual is not None else dropped
        return bb.ln_f(residual.to(dtype=bb.ln_f.weight.dtype))

    def _aligned_length(self, input_ids):
        """Round 6: several sequences of a length that is not a multiple of 64 -- the reference trainer's own batches: L = max_length - 1
        (hg38_dataset.py:222), B = 256 / 8 / 2 (hg38_hyena.yaml:47-48) -- run on sequences padded at the END to the next multiple of 64.  Every
        operation of the model is causal or per-position (embedding, LayerNorm, MLP, short conv, long conv, gates), so positions < L see exactly the
        values of the unpadded run (the long convolution may pick a different transform size: fp32 rounding level); the pad positions' logits
        are dropped before anybody sees them, so they receive zero gradients and contribute nothing to any weight gradient.  What it buys: inside a
        channel row of the flattened (C, B L) layout the rows of odd-length sequences start 2 bytes off every 4 / 16-byte boundary -- one layer at
        32767 x 8 ran 11 % slower than at 32768 x 8, the step at 1023 x 256 x 128 6 % slower (profiles/r6a_bench_default.json).  Only when every
        layer's l_max admits the padded length (hg38 configurations: l_max = max_length + 2) and the fused kernels are in use -- and only for a
        CAUSAL stack: a bidirectional filter (HyenaFilter(bidirectional=True)) centres the input in a 2 L window, so the padded length moves every
        output; a mixer that is not a HyenaOperator is not known to be causal.  Such models run at the length they are given."""
        return self._aligned_total(input_ids.shape[0], input_ids.shape[1], input_ids.is_cuda)

    def _aligned_total(self, B, L, on_device):
        """``_aligned_length``'s rule for B sequences of L positions in all (with a soft prefix: n + L)"""
        # ONE odd-length sequence: its rows are aligned (pitched), what is left are the library weight-gradient products over an odd number of
        # positions (2^20 - 1: dW1 712 vs 612 us, dW_in 611 vs 571, dW_out 303 vs 260 per layer: profiles/r6_wgrad_plan.txt).  Padded where that
        # turns them into the aligned one-level plan -- the padded length a multiple of 4096 (2^20 - 1, 32767: model step 157.5 -> 156.3 ms at
        # 2^20 - 1); at 999 999 / 449 999 the padded count still needs the two-level plan and padding bought nothing (profiles/r6aa_*)
        if not PAD_SEQUENCES or L % _SEQ_ALIGN == 0 or L < _SEQ_ALIGN:
            return L
        if B <= 1 and (L < _PAD_SINGLE_MIN or (L + (-L) % _SEQ_ALIGN) % _PAD_SINGLE_ROWS != 0):
            return L
        from . import _lib
        if not (on_device or _lib._backend.name != "hip"):
            return L
        Lp = L + (-L) % _SEQ_ALIGN
        emb = self.backbone.embeddings
        if emb.max_position_embeddings > 0 and Lp > emb.max_position_embeddings:
            return L
        from .hyena import HyenaOperator
        for mixer in self._mixers():
            if not isinstance(mixer, HyenaOperator) or getattr(mixer.filter_fn, "bidirectional", False):
                return L
            if mixer.l_max < Lp:
                return L
        return Lp

    def hidden_at(self, input_ids, positions=None, soft_tokens=None, soft_dropout_p=0.0, soft_fused=True):
        """the final norm's output (B, n_pos, D) at ``positions``, an (n_pos,) int64 index into the L INPUT positions shared by the batch (None: all
        of them); soft positions are never returned.  (hidden, residual) are gathered in front of drop_f / ln_f: the norm and whatever head
        follows are per-position, so they run on B n_pos rows instead of B (n + L) and give the rows of the full computation.  The end-padding
        rule of ``_aligned_length`` applies to the total n + L: pad ids are appended, their positions dropped here."""
        if positions is None:
            # all positions: the norm runs over the n + L (+ pad) rows as they lie and its output is sliced -- a view; cutting the soft rows
            # out in front of it would copy B L D elements of hidden and of the residual, and scatter as many in the backward
            normed, n = self._hidden_all(input_ids, soft_tokens, soft_dropout_p, soft_fused)
            return normed[:, n:n + input_ids.shape[1]]
        if positions.dim() != 1 or positions.dtype != torch.int64:
            raise ValueError("positions has to be an (n_pos,) int64 index")
        hidden_states, residual, n = self._trunk_padded(input_ids, soft_tokens, soft_dropout_p, soft_fused)
        idx = positions.to(hidden_states.device) + n
        return self._final_norm(hidden_states.index_select(1, idx), residual.index_select(1, idx))

    def _trunk_padded(self, input_ids, soft_tokens, soft_dropout_p, soft_fused):
        """(hidden_states, residual, n) of ``trunk`` over the n soft + L input positions, end-padded by ``_aligned_total``'s rule"""
        B, L = input_ids.shape
        n = 0 if soft_tokens is None else soft_tokens.shape[0]
        Tp = self._aligned_total(B, n + L, input_ids.is_cuda)
        ids = F.pad(input_ids, (0, Tp - n - L), value=0) if Tp != n + L else input_ids
        return self.trunk(ids, soft_tokens=soft_tokens, soft_dropout_p=soft_dropout_p, soft_fused=soft_fused) + (n,)

    def _hidden_all(self, input_ids, soft_tokens=None, soft_dropout_p=0.0, soft_fused=True):
        """(final norm's output over ALL rows (B, n + L + pad, D), n): the input positions are [:, n:n + L]"""
        hidden_states, residual, n = self._trunk_padded(input_ids, soft_tokens, soft_dropout_p, soft_fused)
        return self._final_norm(hidden_states, residual), n

    def _mixers(self):
        return [getattr(blk.mixer, "layer", blk.mixer) for blk in self.backbone.layers]      # (a CheckpointedModule is unwrapped)

    def allocate_inference_cache(self, batch_size, max_seqlen, dtype=None, fan=1, prompt_len=None, lookahead=None, **kwargs):
        """{layer key: HyenaDecodeState} for InferenceParams.key_value_memory_dict (flash_attn's generate assigns it that way).  Every layer must
        be servable (HyenaOperator._forward_cached's refusals apply here, up front).  The caches are snapshots of the weights at this call.
        ``fan`` / ``prompt_len``: batch_size = G fan rows continue G prompts of prompt_len positions; ``lookahead``: every layer's step reads
        a carry taken once per W positions, not its whole history (``HyenaOperator.allocate_inference_cache``)."""
        return {m._decode_key(): m.allocate_inference_cache(batch_size, max_seqlen, dtype=dtype, fan=fan, prompt_len=prompt_len,
                                                            lookahead=lookahead)
                for m in self._mixers()}

    def reorder_inference_cache(self, inference_params, parents):
        """``_reorder_cache``: every layer's decode cache continues row b as what row ``parents[b]`` was (``HyenaDecodeState.reorder``:
        device int32 (B,), parents within b's fan group; fan-out caches only).  Every layer is checked before any of them moves."""
        states = list(inference_params.key_value_memory_dict.values())
        for s in states:
            if s.fan == 1 or s.ragged or s.W:
                s.reorder(parents)                     # raises
        for s in states:
            s.reorder(parents)

    def forward(self, input_ids, position_ids=None, inference_params=None, state=None):
        # (the head through projection.hyena_linear: its weight gradient contracts 16 x 256 outputs over 10^6 tokens, which the GEMM library
        # runs on 16 workgroups -- 1.19 ms per step at 2^20 tokens, profiles/r4y_model_stats.csv -- and the split-K form does not)
        if inference_params is not None:
            # incremental decoding: the prompt as it is (padding would put positions into the cache), then one position per call -- or
            # with inference_params.allow_append (B, T) known tokens at an offset, which every layer appends in block steps
            # (HyenaOperator._forward_cached)
            emb = self.backbone.embeddings
            if position_ids is None and emb.max_position_embeddings > 0:
                off = int(inference_params.seqlen_offset)
                position_ids = torch.arange(off, off + input_ids.shape[1], dtype=torch.long, device=input_ids.device)
            hidden = self.hidden(input_ids, position_ids, inference_params=inference_params)
            lm_logits = hyena_linear(hidden, self.lm_head.weight, self.lm_head.bias)
            return namedtuple("CausalLMOutput", ["logits"])(logits=lm_logits), None
        L = input_ids.shape[1]
        Lp = self._aligned_length(input_ids) if position_ids is None else L
        if Lp != L:
            input_ids = F.pad(input_ids, (0, Lp - L), value=0)     # any valid token id: the pad positions' outputs are dropped
        lm_logits = hyena_linear(self.hidden(input_ids, position_ids), self.lm_head.weight, self.lm_head.bias)
        if Lp != L:
            lm_logits = lm_logits[:, :L]                 # (a view: the pad positions' logits reach nobody -> zero gradients)
        return namedtuple("CausalLMOutput", ["logits"])(logits=lm_logits), None

    @torch.no_grad()
    def score_continuations(self, context_ids, continuations, vocab_size=None, return_logits=False):
        """log-likelihood of n candidate continuations of T tokens after each of G contexts of P tokens:
        ``context_ids`` (G, P), ``continuations`` (G, n, T) -> ``logprobs`` (G, n, T) fp32 with
        ``logprobs[g, j, i] = log p(continuations[g, j, i] | context_ids[g], continuations[g, j, :i])``.

        One prefill over the G contexts fills a decode cache laid out for n rows per context (``fan=n``: the history below
        ``(P // 8192) * 8192`` is kept once per context); token 0 of every candidate is scored from its context's last logits; one cached
        forward over ``continuations[..., :-1]`` as (G n, T - 1) then appends the known tokens in block steps of at most 64 positions, each
        streaming the history once (``HyenaDecodeState.step_block``).  ``vocab_size``: the softmax runs over the first ``vocab_size`` logit
        columns (the padded vocabulary excluded; None: all).  ``return_logits=True``: also the (G, n, T, V) fp32 logits."""
        if context_ids.dim() != 2 or continuations.dim() != 3 or continuations.shape[0] != context_ids.shape[0]:
            raise ValueError(f"score_continuations takes context_ids (G, P) and continuations (G, n, T) (got {tuple(context_ids.shape)} and "
                             f"{tuple(continuations.shape)})")
        (G, P), (_, n, T) = context_ids.shape, continuations.shape
        if G < 1 or P < 1 or n < 1 or T < 1:
            raise ValueError(f"score_continuations needs at least one context, context token, candidate and continuation token "
                             f"(got G = {G}, P = {P}, n = {n}, T = {T})")
        from . import _lib
        from .inference import InferenceParams
        limit = min([getattr(m, "l_max", _lib.MAX_L) for m in self._mixers()] + [_lib.MAX_L])
        if P + T - 1 > limit:
            raise ValueError(f"context ({P}) + continuation ({T}) - 1 = {P + T - 1} positions do not fit the decode cache's limit of {limit}")
        if continuations.dtype != context_ids.dtype or continuations.device != context_ids.device:
            raise ValueError("context_ids and continuations must have the same dtype and device")
        Vall = self.lm_head.weight.shape[0]
        V = Vall if vocab_size is None else int(vocab_size)
        if not 1 <= V <= Vall:
            raise ValueError(f"vocab_size={vocab_size}: the model has {Vall} logit columns")
        if int(continuations.min()) < 0 or int(continuations.max()) >= V:
            raise ValueError(f"continuations hold token ids outside [0, {V})")
        B = G * n
        ip = InferenceParams(max_seqlen=P + T - 1, max_batch_size=B, allow_append=True)
        ip.key_value_memory_dict = self.allocate_inference_cache(B, P + T - 1, **({} if n == 1 else dict(fan=n, prompt_len=P)))
        first = self(context_ids, inference_params=ip)[0].logits[:, -1:].float()                     # (G, 1, V)
        logits = first[:, None].expand(G, n, 1, first.shape[-1])
        if T > 1:
            ip.seqlen_offset = P
            rest = self(continuations[:, :, :-1].reshape(B, T - 1), inference_params=ip)[0].logits.float()
            logits = torch.cat([logits, rest.view(G, n, T - 1, -1)], dim=2)
        logits = logits.contiguous()                                                                  # (G, n, T, V)
        logprobs = torch.log_softmax(logits[..., :V], dim=-1).gather(-1, continuations.long().unsqueeze(-1)).squeeze(-1)
        return (logprobs, logits) if return_logits else logprobs

    # ---- variant effect scoring: one reference pass, edited windows on device (hyena_dna_amd/variants.py) ---------------------------------
    def _check_edit_windows(self, ref_ids, positions, groups, T, what="T"):
        """the refusals every edited-window entry point shares, before any work -> (G, L, M, groups)"""
        from . import _lib
        from .inference import check_decodable
        if self.backbone.embeddings.max_position_embeddings > 0:
            raise NotImplementedError("edited windows need a model without learned position embeddings (max_position_embeddings = 0): a "
                                      "window row would need its absolute position's embedding")
        if not torch.is_tensor(ref_ids) or ref_ids.dim() != 2 or ref_ids.dtype != torch.int64 or ref_ids.shape[0] < 1 or ref_ids.shape[1] < 1:
            raise ValueError("ref_ids has to be a (G >= 1, L >= 1) int64 tensor of token ids")
        G, L = ref_ids.shape
        if not 1 <= int(T) <= _lib.VARIANT_TMAX:
            raise ValueError(f"{what}={T}: a window holds 1 ... {_lib.VARIANT_TMAX} positions")
        if not torch.is_tensor(positions) or positions.dim() != 1 or positions.dtype != torch.int64 or positions.shape[0] < 1:
            raise ValueError("positions has to be an (M >= 1,) int64 tensor")
        if positions.device != ref_ids.device:
            raise ValueError(f"positions live on {positions.device}, ref_ids on {ref_ids.device}")
        M = positions.shape[0]
        if groups is None:
            if G != 1:
                raise ValueError(f"groups is required with {G} reference rows: the row of every variant")
            groups = torch.zeros_like(positions)
        if not torch.is_tensor(groups) or groups.shape != (M,) or groups.dtype != torch.int64 or groups.device != ref_ids.device:
            raise ValueError(f"groups has to be an ({M},) int64 tensor on {ref_ids.device}")
        for m in self._mixers():
            if not hasattr(m, "_forward_edit_windows"):
                raise NotImplementedError(f"edited windows are served by HyenaOperator mixers only (got {type(m).__name__})")
            check_decodable(m, max_seqlen=L)
        if int(positions.min()) < 0 or int(positions.max()) >= L:
            raise ValueError(f"positions hold entries outside [0, {L})")
        if int(groups.min()) < 0 or int(groups.max()) >= G:
            raise ValueError(f"groups hold entries outside [0, {G})")
        return G, L, M, groups

    @torch.no_grad()
    def forward_edited_windows(self, ref_ids, positions, window_tokens, groups=None, max_window_tokens=None):
        """``ref_ids`` (G, L), ``positions`` (M,), ``window_tokens`` (M, T) -> ``(ref_logits (G, L, V), logits (M, T, V))``:
        ``logits[m, i]`` is the model's logits at position ``positions[m] + i`` of the sequence that equals ``ref_ids[groups[m]]`` with
        positions ``[positions[m], positions[m] + T)`` replaced by ``window_tokens[m]``; rows with ``positions[m] + i >= L`` are zeros.

        ONE forward over the reference (the cached prefill's route: ``ref_logits`` are its logits bit for bit) serves all M edits; every
        edit then costs T positions through the per-position layers and a T x T triangular product per channel and layer -- exact, because
        the long convolution is linear in its input (hyena_dna_amd/variants.py).  Nothing of the result beyond ``positions[m] + T - 1`` is
        computed.  ``groups`` (M,): the reference row of every edit (None with G = 1).  ``max_window_tokens``: the window pass runs
        ``max(1, max_window_tokens // T)`` windows at a time, which bounds its activations; the kept reference windows are 6 M T d_model
        bytes per layer (2-byte I/O) whatever it is.  All ids int64 on the model's device; 1 <= T <= 1024."""
        from .variants import EditWindowParams
        if not torch.is_tensor(window_tokens) or window_tokens.dim() != 2 or window_tokens.dtype != torch.int64:
            raise ValueError("window_tokens has to be an (M, T) int64 tensor of token ids")
        T = window_tokens.shape[1]
        G, L, M, groups = self._check_edit_windows(ref_ids, positions, groups, T, what="window_tokens' T")
        if window_tokens.shape[0] != M or window_tokens.device != ref_ids.device:
            raise ValueError(f"window_tokens has to be ({M}, T) on {ref_ids.device} (got {tuple(window_tokens.shape)} on {window_tokens.device})")
        per = M if max_window_tokens is None else max(1, int(max_window_tokens) // T)
        if max_window_tokens is not None and int(max_window_tokens) < 1:
            raise ValueError(f"max_window_tokens={max_window_tokens}: at least one token")
        ew = EditWindowParams(positions, groups, T)
        ref_logits = self(ref_ids, inference_params=ew)[0].logits
        ew.phase = "window"
        outs = []
        for lo in range(0, M, per):
            hi = min(lo + per, M)
            ew.select(lo, hi)
            outs.append(self(window_tokens[lo:hi], inference_params=ew)[0].logits)
        logits = outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)
        past = (positions[:, None] + torch.arange(T, device=positions.device)[None, :]) >= L
        return ref_logits, logits.masked_fill(past[:, :, None], 0)

    @torch.no_grad()
    def score_variants(self, ref_ids, positions, alts, groups=None, horizon=64, vocab_size=None, max_window_tokens=None):
        """Zero-shot effect of M single-base substitutions: ``ref_ids`` (G, L), ``positions`` (M,) with 1 <= positions[m] <= L - 1,
        ``alts`` (M,) the substituted token -> ``VariantScores(site, downstream, llr, complete)``, log-likelihood differences (alt - ref)
        under the model, with lsm = log_softmax over the first ``vocab_size`` logit columns (None: all), g = groups[m], p = positions[m],
        T = ``horizon``:

            site[m]          = lsm(ref_logits[g, p - 1])[alt] - lsm(ref_logits[g, p - 1])[ref[p]]
            downstream[m, i] = lsm(logits[m, i])[ref[p + i + 1]] - lsm(ref_logits[g, p + i])[ref[p + i + 1]]     for p + i + 1 <= L - 1, else 0
            llr[m]           = site[m] + downstream[m].sum()
            complete[m]      = p + T >= L - 1

        ``logits`` are ``forward_edited_windows``' over the window tokens ``[alt, ref[p + 1], ..., ref[p + T - 1]]``.  Where ``complete`` holds,
        ``llr`` is the log-likelihood ratio of the whole sequences; elsewhere it is TRUNCATED at the horizon: the terms of positions past
        p + T are left out (they decay with the filter but are not zero).  1 <= horizon <= 1024."""
        T = int(horizon)
        G, L, M, groups = self._check_edit_windows(ref_ids, positions, groups, T, what="horizon")
        if not torch.is_tensor(alts) or alts.shape != (M,) or alts.dtype != torch.int64 or alts.device != ref_ids.device:
            raise ValueError(f"alts has to be an ({M},) int64 tensor on {ref_ids.device}")
        Vall = self.lm_head.weight.shape[0]
        V = Vall if vocab_size is None else int(vocab_size)
        if not 1 <= V <= Vall:
            raise ValueError(f"vocab_size={vocab_size}: the model has {Vall} logit columns")
        if int(positions.min()) < 1:
            raise ValueError(f"positions hold entries outside [1, {L - 1}]: a substitution at position 0 has no context to be scored from")
        if int(alts.min()) < 0 or int(alts.max()) >= V:
            raise ValueError(f"alts hold token ids outside [0, {V})")
        if int(ref_ids.min()) < 0 or int(ref_ids.max()) >= V:
            raise ValueError(f"ref_ids hold token ids outside [0, {V})")
        dev = ref_ids.device
        idx = positions[:, None] + torch.arange(T + 1, device=dev)[None, :]                       # (M, T + 1): p ... p + T
        ref_tok = ref_ids[groups[:, None], idx.clamp(max=L - 1)]                                  # ref[p + j], clipped past the end
        window = torch.cat([alts[:, None], ref_tok[:, 1:T]], dim=1)
        ref_logits, logits = self.forward_edited_windows(ref_ids, positions, window, groups=groups, max_window_tokens=max_window_tokens)
        # the reference's rows p - 1 ... p + T - 1, gathered before the softmax: M (T + 1) rows, not G L
        rows = ref_logits[groups[:, None], (idx - 1).clamp(max=L - 1)][..., :V].float()           # (M, T + 1, V)
        lsm_ref = torch.log_softmax(rows, dim=-1)
        lsm_alt = torch.log_softmax(logits[..., :V].float(), dim=-1)                              # (M, T, V)
        site = (lsm_ref[:, 0].gather(-1, alts[:, None]) - lsm_ref[:, 0].gather(-1, ref_tok[:, :1])).squeeze(-1)
        nxt = ref_tok[:, 1:, None]                                                                # ref[p + i + 1], i < T
        down = (lsm_alt.gather(-1, nxt) - lsm_ref[:, 1:].gather(-1, nxt)).squeeze(-1)
        down = down.masked_fill(idx[:, 1:] > L - 1, 0)
        VariantScores = namedtuple("VariantScores", ["site", "downstream", "llr", "complete"])
        return VariantScores(site=site, downstream=down, llr=site + down.sum(-1), complete=positions + T >= L - 1)

    @torch.no_grad()
    def saturation_mutagenesis(self, ref_ids, start, stop, alphabet=(7, 8, 9, 10), horizon=64, vocab_size=None, max_window_tokens=None):
        """``score_variants``' ``llr`` of every substitution of ``alphabet`` at every position of ``[start, stop)`` of ONE reference
        ``ref_ids`` (L,) -> (stop - start, len(alphabet)) fp32; the reference base's own entry is exactly 0.  1 <= start < stop <= L.
        One ``score_variants`` call over (stop - start) len(alphabet) variants (position-major), so its other entries are that call's."""
        if not torch.is_tensor(ref_ids) or ref_ids.dim() != 1 or ref_ids.dtype != torch.int64:
            raise ValueError("ref_ids has to be an (L,) int64 tensor: saturation_mutagenesis takes one reference")
        L = ref_ids.shape[0]
        start, stop = int(start), int(stop)
        if not 1 <= start < stop <= L:
            raise ValueError(f"start={start}, stop={stop}: positions 1 <= start < stop <= {L}")
        alphabet = [int(a) for a in alphabet]
        if len(alphabet) < 1:
            raise ValueError("alphabet holds no token")
        A = len(alphabet)
        pos = torch.arange(start, stop, device=ref_ids.device).repeat_interleave(A)
        alts = torch.tensor(alphabet, dtype=torch.int64, device=ref_ids.device).repeat(stop - start)
        llr = self.score_variants(ref_ids[None], pos, alts, horizon=horizon, vocab_size=vocab_size, max_window_tokens=max_window_tokens).llr
        return llr.masked_fill(alts == ref_ids[pos], 0).view(stop - start, A)

    def loss(self, input_ids, targets, ignore_index=-100):
        """next-token cross entropy (src/tasks/metrics.py cross_entropy over the flattened logits), logits in fp32"""
        logits = self.forward(input_ids)[0].logits
        return token_cross_entropy(logits, targets, ignore_index=ignore_index)


def token_cross_entropy(logits, targets, ignore_index=-100):
    """``F.cross_entropy(logits.float().reshape(-1, V), targets.reshape(-1), ignore_index=ignore_index)`` -- the mean of -log p[target] over
    the tokens that are not ignored -- written as log-softmax + gather + masked mean.  Same value and gradients to fp32 summation order; on
    ROCm PyTorch's own reduction for this 2-D case (nll_loss_forward_reduce_cuda_kernel_2d) runs in ONE workgroup: 1.07 ms forward and 0.8 ms
    backward per step at 2^20 tokens x 16 classes (profiles/r4y_model_stats.csv) for 64 MB of logits; these are streaming kernels."""
    lp = torch.log_softmax(logits.float().reshape(-1, logits.shape[-1]), dim=-1)
    t = targets.reshape(-1)
    valid = t != ignore_index
    picked = lp.gather(1, t.clamp_min(0).unsqueeze(1)).squeeze(1)
    return -(picked * valid).sum() / valid.sum()


class CheckpointedModule(nn.Module):
    """long_conv_lm.py:39-45: the wrapped module under the attribute `layer`, its forward recomputed in the backward."""

    def __init__(self, layer):
        super().__init__()
        self.layer = layer

    def forward(self, x, **kwargs):
        if kwargs.get("inference_params") is not None:        # inference: nothing to recompute, the wrapped module runs as it is
            return self.layer(x, **kwargs)
        from torch.utils.checkpoint import checkpoint
        return checkpoint(self.layer, x, use_reentrant=False)


class GraphedTrainStep:
    """One whole training step -- forward, loss, backward, optimizer step -- captured into ONE hipGraph and replayed.

    Below L ~ 32k the eager step of the 8-layer model is bound by the ~1 500 kernel launches Python issues, not by the GPU
    (DESIGN.md section 5); a replay costs one launch.  Everything on this path is stream-ordered and allocation-free after the
    warm-up (include/hyena_fftconv.h), so the capture needs nothing special: static input buffers, gradients that live inside
    the graph's memory pool, and an optimizer built with ``capturable=True`` (its step counters are device tensors).

        opt  = torch.optim.AdamW(model.parameters(), lr=6e-4, weight_decay=0.1, capturable=True)
        step = GraphedTrainStep(model, opt, input_ids, targets)      # warms up (3 eager steps) and captures
        loss = step(next_ids, next_targets)                           # copies into the static buffers, replays

    The captured step always sees batches of the captured shape; to change the learning rate between replays make it a
    device tensor (``lr=torch.tensor(6e-4, device=...)``) and update it in place.  Drop the loss / outputs of earlier eager
    steps before constructing this (their autograd graphs pin gradient accumulators to another stream), and see
    ``hyena_dna_amd/__init__.py`` for the ROCm runtime setting whole-step replays need (applied at import).
    """

    def __init__(self, model, optimizer, input_ids, targets, autocast_dtype=torch.bfloat16, warmup=3, ignore_index=-100,
                 clip_grad_norm=0.0):
        if not input_ids.is_cuda:
            raise RuntimeError("GraphedTrainStep captures a hipGraph: model and batch must live on a ROCm device")
        for group in optimizer.param_groups:
            if not group.get("capturable", False):
                raise RuntimeError("GraphedTrainStep needs an optimizer built with capturable=True")
        import hyena_dna_amd
        if not hyena_dna_amd.GRAPH_SAFE or os.environ.get("DEBUG_CLR_GRAPH_PACKET_CAPTURE") != "0":
            raise RuntimeError("GraphedTrainStep: hipGraph replays of a whole step are only reliable on this ROCm runtime with "
                               "DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 in the environment before the HIP runtime initialises "
                               "(call hyena_dna_amd.prepare_graph_runtime() before the first torch.cuda call, or export the "
                               "variable; a process that exported it at start-up but touched torch.cuda before importing this package says so "
                               "with HYENA_GRAPH_SAFE_OVERRIDE=1); see hyena_dna_amd/__init__.py and INTEGRATION.md section 6")
        self.model, self.optimizer = model, optimizer
        self.ids, self.targets = input_ids.clone(), targets.clone()
        self.autocast_dtype, self.ignore_index = autocast_dtype, ignore_index
        self.clip_grad_norm = float(clip_grad_norm or 0.0)           # trainer.gradient_clip_val (hg38_hyena.yaml:41), inside the graph
        # Gradient-accumulation nodes remember the stream they were created on.  Nodes left over from eager steps on another
        # stream (kept alive by a retained loss tensor, or by not-yet-collected reference cycles of autograd contexts) would run
        # OUTSIDE the capture: drop them, and warm up on the very stream the capture uses.
        import gc
        gc.collect()
        from . import _lib
        # keep-the-spectra decisions are re-taken during this warm-up, with the model (and, from its second step on, the optimizer state)
        # already allocated -- not inherited from whatever memory was free when a shape was first seen; they then stay fixed for the capture
        _lib.reset_save_decisions(input_ids.device)
        side = torch.cuda.Stream(input_ids.device)
        self._side = side
        side.wait_stream(torch.cuda.current_stream(input_ids.device))
        with torch.cuda.stream(side):                 # twiddle tables, workspaces, optimizer state, GEMM heuristics: all created here
            # The warm-up runs REAL optimizer updates (the optimizer's state tensors must exist, on this stream, before the capture).  They
            # are not training steps: parameters, Adam moments and step counters are put back afterwards, in place (the graph will hold
            # these very tensors), so that a graphed run and an eager run of the same config + seed start from the same state.
            params = [p for g in optimizer.param_groups for p in g["params"]]
            with torch.no_grad():
                snap_p = [p.detach().clone() for p in params]
            had_state = {id(p): {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in optimizer.state.get(p, {}).items()}
                         for p in params}
            for _ in range(max(1, int(warmup))):
                optimizer.zero_grad(set_to_none=True)
                self._fwd_bwd()
                optimizer.step()
            optimizer.zero_grad(set_to_none=True)      # the gradients of the captured step live in the graph's pool
            with torch.no_grad():
                for p, q in zip(params, snap_p):
                    p.copy_(q)
                for p in params:
                    st, old = optimizer.state.get(p, {}), had_state[id(p)]
                    for k, v in st.items():
                        if torch.is_tensor(v):
                            if k in old and torch.is_tensor(old[k]):
                                v.copy_(old[k])
                            else:
                                v.zero_()                  # fresh optimizer: moments and the step counter start at zero
            del snap_p, had_state
            gc.collect()
            side.synchronize()
            from . import _castcache
            _castcache.invalidate()                    # the batched weight cast becomes part of the captured step
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=side):
                self.loss = self._fwd_bwd().detach()
                optimizer.step()
        torch.cuda.current_stream(input_ids.device).wait_stream(side)

    def release(self):
        """Drop the graph and what the long-convolution binding keeps for its capture stream (workspace, tables stay: they are per length).
        Call before building the next GraphedTrainStep of a sequence-length stage."""
        from . import _castcache, _lib
        dev = self.ids.device
        self.graph = None
        self.loss = None
        torch.cuda.synchronize(dev)
        _castcache.invalidate()                        # the shadows hold the weights of BEFORE the last replay's update (see __call__)
        _lib.release_stream_state(dev, self._side.cuda_stream)
        self._side = None

    def _fwd_bwd(self):
        enabled = self.autocast_dtype is not None and self.autocast_dtype != torch.float32
        with torch.autocast("cuda", dtype=self.autocast_dtype if enabled else torch.bfloat16, enabled=enabled):
            loss = self.model.loss(self.ids, self.targets, ignore_index=self.ignore_index)
        loss.backward()
        if self.clip_grad_norm > 0:                                   # device-side norm and scale: no host sync, capturable
            torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.clip_grad_norm)
        return loss

    def __call__(self, input_ids=None, targets=None):
        """Replays the step on (input_ids, targets) -- or on the batch already in the static buffers -- and returns the
        (static, device-resident) loss tensor; read it with .item() only when you need the number."""
        if input_ids is not None:
            self.ids.copy_(input_ids, non_blocking=True)
        if targets is not None:
            self.targets.copy_(targets, non_blocking=True)
        self.graph.replay()
        # The replay refreshed the 16-bit weight shadows (the refresh is part of the captured step) and THEN updated the parameters, on the
        # device: neither their version counters nor their addresses moved, so to _castcache the shadows look fresh while they are one
        # optimizer step old.  Host-only (a loop over the entries, nothing is launched): eager work between two replays casts again.
        from . import _castcache
        _castcache.invalidate()
        return self.loss


class GraphedDecodeStep:
    """The whole per-token step of cached generation -- embedding of a static (B, 1) token buffer, every layer's decode step, ln_f, the
    head -- captured into ONE hipGraph after the prefill and replayed once per token (``generate(use_cache=True, cg=True)``).  At short
    contexts the eager step is a few dozen launches of almost no work each; a replay is one.  The decode kernels read the position from
    device memory (one for the batch, or one per row after a prefill with ``lengths_per_sample``), so the one graph serves every position;
    sampling stays outside -- unless a ``sampler`` (``inference.DeviceSampler``) is given: then the graph ends with the sampling kernel, which
    writes the next step's tokens into the static id buffer itself, and a token is ``step.replay()`` and nothing else.

        step = GraphedDecodeStep(model, ip, batch_size)      # after the prefill: warms up on the capture stream, captures
        logits = step(next_tokens)                           # (B, V) static buffer, overwritten by the next replay
        step.release()

    Warm-up steps run the real kernels: the cache's tail state and position (and the sampler's columns, done flags and the sequence columns
    it wrote) are put back afterwards (the history column they wrote is rewritten by the first replay).  Same preconditions as
    ``GraphedTrainStep`` (``hyena_dna_amd.prepare_graph_runtime()``)."""

    def __init__(self, model, inference_params, batch_size, warmup=2, sampler=None):
        import hyena_dna_amd
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("GraphedDecodeStep captures a hipGraph: the model must live on a ROCm device")
        if not hyena_dna_amd.GRAPH_SAFE or os.environ.get("DEBUG_CLR_GRAPH_PACKET_CAPTURE") != "0":
            raise RuntimeError("GraphedDecodeStep: hipGraph replays are only reliable on this ROCm runtime with DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 "
                               "in the environment before the HIP runtime initialises (hyena_dna_amd.prepare_graph_runtime(); INTEGRATION.md "
                               "section 6)")
        self.model, self.ip, self.sampler = model, inference_params, sampler
        self.ids = torch.zeros(batch_size, 1, dtype=torch.long, device=dev)
        emb = model.backbone.embeddings
        self.pos_ids = torch.zeros(1, dtype=torch.long, device=dev) if emb.max_position_embeddings > 0 else None
        states = list(inference_params.key_value_memory_dict.values())
        # lookahead caches: the graph holds the step only.  From here on their steps neither refresh nor count (a warm-up step past the
        # window is parked by the kernels; ``base``, the carry and the host counters stay as they are) and every replay is preceded by
        # ``la_before_step`` on the current stream: the refresh when one is due, and the count.
        self._la = [s for s in states if getattr(s, "W", 0)]
        for s in self._la:
            s.la_external = True
        try:
            side = torch.cuda.Stream(dev)
            self._side = side
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                snap = [(s.tail.clone(), s.pos.clone(), s.pos_rows.clone()) for s in states]
                restore_sampler = sampler.snapshot(max(1, int(warmup))) if sampler is not None else None
                for _ in range(max(1, int(warmup))):
                    self._run()
                for s, (tail, pos, pos_rows) in zip(states, snap):
                    s.tail.copy_(tail)
                    s.pos.copy_(pos)
                    s.pos_rows.copy_(pos_rows)
                if restore_sampler is not None:
                    restore_sampler()
                side.synchronize()
                self.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph, stream=side):
                    self.logits = self._run()
            torch.cuda.current_stream(dev).wait_stream(side)
        except BaseException:
            # no graph came of it: the caches go back to the eager schedule (an eager step() refreshes and counts again)
            for s in self._la:
                s.la_external = False
            raise

    def _run(self):
        out = self.model(self.ids, position_ids=self.pos_ids, inference_params=self.ip)
        logits = out[0].logits[:, -1]
        if self.sampler is not None:
            self.sampler(logits, self.ids)
        return logits

    def __call__(self, input_ids):
        """replays the step for the tokens input_ids (B, 1) at position ip.seqlen_offset; returns the static (B, V) logits"""
        self.ids.copy_(input_ids, non_blocking=True)
        if self.pos_ids is not None:
            self.pos_ids.fill_(int(self.ip.seqlen_offset))
        for s in self._la:
            s.la_before_step()
        self.graph.replay()
        return self.logits

    def replay(self):
        """with a sampler: the step for the tokens the previous replay (or an eager sampler call on ``ids``) left in the id buffer"""
        if self.pos_ids is not None:
            self.pos_ids.fill_(int(self.ip.seqlen_offset))
        for s in self._la:
            s.la_before_step()
        self.graph.replay()

    def release(self):
        if self.graph is None:
            return
        from . import _lib
        dev = self.ids.device
        for s in self._la:
            s.la_external = False
        self.graph = None
        self.logits = None
        torch.cuda.synchronize(dev)
        _lib.release_stream_state(dev, self._side.cuda_stream)
        self._side = None
