"""Incremental decoding: the per-layer cache of ``HyenaOperator`` and flash_attn's ``InferenceParams``.

Every operation of the HyenaDNA model is per-position or causal, and the implicit filter is prefix-consistent (``PositionalEmbedding`` slices
one ``l_max``-long table), so position t of a layer's long convolution is ``sum_{s <= t} k[c, t - s] vg[b, c, s] + fb[c] vg[b, c, t]``: a
dot product over the history of the convolution's input ``vg = v * x1``.  ``HyenaDecodeState`` holds what that takes -- the filter
``filter_dl(max_seqlen)``, the history, the last two in_proj outputs the 3-tap short convolution still needs, the position (in device
memory: one captured graph serves every position; one int for the batch, or one per row after a right-padded prefill with
``InferenceParams.lengths_per_sample``) and the step's small buffers -- and ``HyenaOperator.forward(u, inference_params=ip)``
fills it with a prefill (``ip.seqlen_offset == 0``) and advances it afterwards by one position per call, or by the T known positions of a
``(B, T, D)`` input in block steps that stream the history once per 64 positions (``step_block``; csrc/decode_kernels.h).  With
``lookahead=W`` a cache takes the history's share of the next W outputs ahead, once per W positions, and a step reads that carry and the
columns written since, not the whole history.
"""
import torch

from . import _lib

__all__ = ["InferenceParams", "HyenaDecodeState", "DeviceSampler", "check_decodable", "check_lookahead", "token_mask", "iupac_constraints",
           "TokenAutomaton", "motif_automaton", "automaton_step_tables"]


class InferenceParams:
    """flash_attn.utils.generation.InferenceParams: ``max_seqlen``, ``max_batch_size``, ``seqlen_offset`` (alias ``sequence_len_offset``, the
    older name), ``batch_size_offset``, ``key_value_memory_dict`` (layer key -> that layer's cache), ``lengths_per_sample``.

    ``lengths_per_sample``: None, or the device int32 (B,) tensor of the prompts' own lengths when the prefill batch is right-padded.  The
    prefill hands it to every layer's cache (``HyenaDecodeState.store_prefill``), which from then on keeps one position per row.

    ``allow_append`` (this package's addition; an attribute set on flash_attn's own object serves as well): with it a call at
    ``seqlen_offset > 0`` with SEVERAL positions per sequence appends them all to the cache in block steps
    (``HyenaDecodeState.step_block``).  Without it such a call stays the error it has always been: a decode loop that hands the model more
    than its one new token by mistake must not move the cache.

    ``lookahead`` (this package's addition): the window W the caches of ``key_value_memory_dict`` were (or are to be) built with
    (``allocate_inference_cache(..., lookahead=W)``; None / 0: none).  Every ``HyenaDecodeState`` keeps its own, which is the one that acts;
    the cached forward of every operator refuses (``ValueError``) a cache whose window is not this one, so the two cannot disagree."""

    def __init__(self, max_seqlen, max_batch_size, seqlen_offset=0, batch_size_offset=0, key_value_memory_dict=None, lengths_per_sample=None,
                 allow_append=False, lookahead=None):
        self.max_seqlen = max_seqlen
        self.max_batch_size = max_batch_size
        self.seqlen_offset = seqlen_offset
        self.batch_size_offset = batch_size_offset
        self.key_value_memory_dict = {} if key_value_memory_dict is None else key_value_memory_dict
        self.lengths_per_sample = lengths_per_sample
        self.allow_append = allow_append
        self.lookahead = check_lookahead(lookahead)

    @property
    def sequence_len_offset(self):
        return self.seqlen_offset

    @sequence_len_offset.setter
    def sequence_len_offset(self, value):
        self.seqlen_offset = value

    def reset(self, max_seqlen, max_batch_size):
        self.max_seqlen = max_seqlen
        self.max_batch_size = max_batch_size
        self.seqlen_offset = 0
        if self.lengths_per_sample is not None:
            self.lengths_per_sample.zero_()


def check_lookahead(lookahead):
    """None / 0 (no lookahead) or a window of 1 ... 64 positions -> the window as an int (0: none)"""
    W = 0 if lookahead is None else int(lookahead)
    if not 0 <= W <= _lib.DECODE_TMAX:
        raise ValueError(f"lookahead={lookahead}: None / 0, or a window of 1 ... {_lib.DECODE_TMAX} positions")
    return W


def check_decodable(op, max_seqlen=None):
    """What the decode step serves: the fused channel-major route of an order-2 causal operator, at most min(l_max, 2^20) positions.
    Anything else is refused here, up front -- never a silent fall-back to recomputing the prefix."""
    from . import hyena as H
    if op.order != 2:
        raise NotImplementedError(f"incremental decoding serves order-2 operators only (this one has order {op.order})")
    if getattr(op.filter_fn, "bidirectional", False):
        raise NotImplementedError("incremental decoding needs a causal filter (bidirectional=True is not causal)")
    if not op._fused_ok() or not H.CHANNEL_MAJOR:
        raise NotImplementedError("incremental decoding serves the fused channel-major operator route only (one head, one block, inner factor 1, "
                                  "3 short-filter taps, no outer mixing / post-order FFN, HYENA_MIXER_LAYOUT=channel)")
    if max_seqlen is not None:
        limit = min(op.l_max, _lib.MAX_L)
        if not 1 <= int(max_seqlen) <= limit:
            raise ValueError(f"max_seqlen={max_seqlen}: the decode cache holds 1 ... {limit} positions (l_max = {op.l_max}, kernel limit 2^20)")


def _default_dtype(op, device):
    dev_type = device.type
    if torch.is_autocast_enabled(dev_type):
        dt = torch.get_autocast_dtype(dev_type)
        if dt in (torch.bfloat16, torch.float16):
            return dt
    return op.in_proj.weight.dtype


class HyenaDecodeState:
    """The decode cache of one order-2 ``HyenaOperator`` for up to ``batch_size`` sequences of up to ``max_seqlen`` positions.

    Like a key-value cache it is a SNAPSHOT of the weights it was built from: the filter ``k = filter_dl(max_seqlen)``, the short filter and
    the biases are copied when the cache is built, the history holds activations of the weights of its time.  Build a new cache after the
    weights change.  ``dtype``: the I/O type of the operator's activations (the autocast type, or the parameters' type); the prefill and
    every step must run in it.

    Memory: k (D, max_seqlen) fp32 + history (batch_size, D, max_seqlen) in ``dtype`` + O(B D) -- at 2^20 x 256 with B = 1 in bf16, 1 GiB
    plus 0.5 GiB per layer.

    ``fan = n > 1``: the batch is G = batch_size / n prompts of ``prompt_len`` positions, each continued n times (row g n + j: sample j of
    prompt g).  The prefill runs over the G prompts; the history below ``S = (prompt_len // 8192) * 8192`` is the same for the n rows of a
    group and is kept once -- ``hist_shared`` (G, D, S) -- and ``hist`` (batch_size, D, max_seqlen - S) holds every row's columns from S
    on.  The step runs the ``_fan`` kernels, whose results equal those of the plain step on the replicated history bit for bit.  A prompt
    shorter than 8192 positions has S = 0: nothing is shared in the step (which is launch-bound there), the prefill is still paid once.

    ``lookahead = W`` (1 ... 64; None / 0: none, and then nothing below exists or runs): the step stops streaming the history.  The
    convolution is linear in it, so a REFRESH at position t0 takes the share of outputs t0 ... t0 + W - 1 that comes from positions below t0
    in one pass over the history (``carry`` (B, W, D) fp32, ``base`` = t0 in device memory), and a step at t in that window reads
    ``carry[:, t - base]`` and the columns base ... t only (``decode_conv_la`` / ``decode_post_la``).  The same sum in another order: the
    results differ from the plain step's by fp32 rounding.  The schedule lives on the host and reads nothing back: a refresh ends
    ``store_prefill``, and ``step`` runs one first whenever the window is used up (``la_used == W``).  A caller that replays captured steps
    (``GraphedDecodeStep``) sets ``la_external`` -- ``step`` then neither refreshes nor counts -- and calls ``la_before_step()`` before
    every replay.  Not with ``fan > 1``, ragged prompts or block steps (follow-ups)."""

    def __init__(self, op, batch_size, max_seqlen, dtype=None, fan=1, prompt_len=None, lookahead=None):
        check_decodable(op, max_seqlen)
        if int(batch_size) < 1:
            raise ValueError(f"batch_size={batch_size}: at least one sequence")
        self.fan = int(fan)
        if self.fan < 1:
            raise ValueError(f"fan={fan}: at least one continuation per prompt")
        self.W = check_lookahead(lookahead)
        if self.W and self.fan > 1:
            raise NotImplementedError("a decode cache with lookahead and fan > 1 (num_return_sequences > 1) is out of scope: the carry serves "
                                      "the plain cache only")
        self.S = 0
        if self.fan > 1:
            if int(batch_size) % self.fan != 0:
                raise ValueError(f"batch_size={batch_size} is not a multiple of fan={fan} (batch_size counts the rows: prompts x fan)")
            if prompt_len is None or not 1 <= int(prompt_len) <= int(max_seqlen):
                raise ValueError(f"prompt_len={prompt_len}: a cache with fan > 1 is laid out for one prompt length in 1 ... max_seqlen = {max_seqlen}")
            self.prompt_len = int(prompt_len)
            self.S = self.prompt_len // _lib.DECODE_CHUNK * _lib.DECODE_CHUNK
        dev = op.in_proj.weight.device
        self.dtype = dtype if dtype is not None else _default_dtype(op, dev)
        if self.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError(f"dtype={self.dtype}: the decode kernels take float32 / bfloat16 / float16 activations")
        self.B, self.L, self.D = int(batch_size), int(max_seqlen), op.d_model
        D, L = self.D, self.L
        with torch.no_grad():
            k = op.filter_fn.filter_dl(L).detach().to(torch.float32)
            if _lib.ld_of(k) is not None and _lib.ld_of(k) % 4 == 0 and k.data_ptr() % 16 == 0 and k.shape == (D, L):
                self.k = k
            else:
                self.k = torch.zeros(D, _lib.row_pitch(L), dtype=torch.float32, device=dev)[:, :L]
                self.k.copy_(k)
            del k
            self.fb = op.filter_fn.conv_bias().detach().to(torch.float32).reshape(D).clone()
            self.bin = op.in_proj.bias.detach().to(torch.float32).clone() if op.in_proj.bias is not None else None
            self.w = op.short_filter.weight.detach().to(torch.float32).reshape(3 * D, 3).clone()
            self.b = op.short_filter.bias.detach().to(torch.float32).clone()
        # fan > 1: columns [0, S) once per group, [S, L) per row (at least one column, so that the row tensor always exists)
        self.hist_shared = torch.zeros(self.B // self.fan, D, _lib.row_pitch(self.S), dtype=self.dtype, device=dev) if self.S > 0 else None
        self.hist = torch.zeros(self.B, D, _lib.row_pitch(max(L - self.S, 1)), dtype=self.dtype, device=dev)
        self.tail = torch.zeros(3 * D, self.B, 2, dtype=torch.float32, device=dev)
        self.pos = torch.zeros(1, dtype=torch.int32, device=dev)
        self.pos_rows = torch.full((self.B,), -1, dtype=torch.int32, device=dev)   # ragged mode (store_prefill(lengths=...)): one position per row
        self.ragged = False
        self.x0 = torch.empty(self.B, D, dtype=torch.float32, device=dev)
        self.z = torch.empty(self.B, D, dtype=self.dtype, device=dev)
        self.part = _lib.decode_partials(self.B, D, L, dev)
        self.block_buf = None                                                         # step_block's part / x0 / z: allocated on first use
        # lookahead: allocated only when asked for
        self.carry = self.carry_part = self.la_part = self.base = None
        self.la_used, self.la_external, self.la_rows = 0, False, self.B
        if self.W:
            self.carry = torch.zeros(self.B, self.W, D, dtype=torch.float32, device=dev)
            self.carry_part = _lib.decode_carry_partials(self.B, D, L, self.W, dev)
            self.la_part = torch.empty(2, self.B, D, dtype=torch.float32, device=dev)
            self.base = torch.zeros(1, dtype=torch.int32, device=dev)                 # (position 0 with a zero carry is a valid window)

    def refresh(self):
        """the carry of the W outputs from the current position on, in one pass over the history (the rows of the last prefill); then
        ``base`` = that position"""
        _lib.decode_carry(self.k, self.hist, self.carry_part, self.carry, self.pos, self.base, self.la_rows, self.L)
        self.la_used = 0

    def la_before_step(self):
        """the host's side of one lookahead step: a refresh first if the window is used up, then one more position counted"""
        if self.la_used >= self.W:
            self.refresh()
        self.la_used += 1

    def store_prefill(self, xT, vg, P, lengths=None):
        """after the prefill forward over P positions: its convolution input vg (B, D, P) and the last two in_proj outputs of xT (3D, B, P).

        ``lengths`` (device int32 (B,), 1 <= lengths[b] <= P): the prompts are right-padded to P and row b really holds lengths[b] positions.
        The model is causal, so everything below lengths[b] is what the unpadded prompt gives; the cache then keeps one position per row
        (``pos_rows``) and ``step`` runs the per-row kernels.  Device work only: nothing here reads ``lengths`` on the host."""
        B = vg.shape[0]
        if self.W and lengths is not None:
            raise NotImplementedError("a decode cache with lookahead keeps one position for the batch: ragged prompts (lengths) with lookahead "
                                      "are out of scope")
        if self.fan > 1:
            if lengths is not None:
                raise NotImplementedError("a decode cache with fan > 1 holds prompts of one length: ragged prompts with fan-out are out of scope")
            G, n, S = self.B // self.fan, self.fan, self.S
            if B != G or P != self.prompt_len:
                raise ValueError(f"this decode cache was built for a prefill of {G} prompts (batch_size / fan) of {self.prompt_len} positions "
                                 f"(got {B} of {P})")
            if S > 0:
                self.hist_shared[:, :, :S].copy_(vg[:, :, :S])
            if P > S:
                self.hist.view(G, n, self.D, -1)[:, :, :, :P - S].copy_(vg[:, None, :, S:P])
            m = min(P, 2)
            self.tail.zero_()
            self.tail.view(-1, G, n, 2)[:, :, :, 2 - m:].copy_(xT[:, :, None, P - m:P])
            self.ragged = False
            self.pos.fill_(P)
            return
        self.hist[:B, :, :P].copy_(vg)
        if lengths is None:
            self.ragged = False
            n = min(P, 2)
            self.tail[:, :B].zero_()
            self.tail[:, :B, 2 - n:].copy_(xT[:, :, P - n:P])
            self.pos.fill_(P)
            if self.W:
                self.la_rows = B
                self.refresh()
            return
        if lengths.shape != (B,) or lengths.dtype != torch.int32 or lengths.device != self.hist.device:
            raise ValueError(f"lengths must be a ({B},) int32 tensor on {self.hist.device} (got {tuple(lengths.shape)} {lengths.dtype} on {lengths.device})")
        self.ragged = True
        # the pad positions' activations go: decode_conv reads up to 7 columns past t_b (times a zero tap) and relies on finite values there
        cols = torch.arange(P, device=lengths.device, dtype=torch.int32)
        self.hist[:B, :, :P].masked_fill_((cols[None, :] >= lengths[:, None])[:, None, :], 0)
        # the tail of row b: columns lengths[b] - 2, lengths[b] - 1 of xT, zeros where they lie before position 0
        idx = lengths.to(torch.int64)[:, None] + torch.tensor([-2, -1], device=lengths.device)            # (B, 2)
        got = xT[:, :, :P].gather(2, idx.clamp(0, P - 1)[None].expand(xT.shape[0], B, 2)).to(torch.float32)
        self.tail[:, :B].copy_(got * (idx >= 0)[None])
        self.pos_rows.fill_(-1)                                                                            # rows past B stay parked
        self.pos_rows[:B].copy_(lengths)

    def step(self, x2):
        """x2 (B, 3D): in_proj output of the new position without bias -> z (B, D) for out_proj (three kernels; advances the position --
        after a prefill with ``lengths``, every row's own)"""
        B = x2.shape[0]
        z = self.z[:B]
        if self.fan > 1:
            if B != self.B:
                raise ValueError(f"a step of a decode cache with fan = {self.fan} takes all {self.B} rows (got {B})")
            _lib.decode_pre_fan(x2, self.bin, self.w, self.b, self.tail, self.hist, self.x0, self.pos, self.L, self.S)
            _lib.decode_conv_fan(self.k, self.hist_shared, self.hist, self.part, self.pos, B, self.fan, self.L, self.S)
            _lib.decode_post_fan(self.part, self.hist, self.fb, self.x0, z, self.pos, B, self.fan, self.L, self.S)
            return z
        if self.ragged:
            _lib.decode_pre_rows(x2, self.bin, self.w, self.b, self.tail, self.hist, self.x0, self.pos_rows, self.L)
            _lib.decode_conv_rows(self.k, self.hist, self.part, self.pos_rows, B, self.L)
            _lib.decode_post_rows(self.part, self.hist, self.fb, self.x0, z, self.pos_rows, B, self.L)
            return z
        if self.W:
            if B > self.la_rows:
                raise ValueError(f"a lookahead step takes at most the {self.la_rows} rows of the prefill (got {B}): the carry covers those")
            if not self.la_external:
                self.la_before_step()
            _lib.decode_pre(x2, self.bin, self.w, self.b, self.tail, self.hist, self.x0, self.pos, self.L)
            _lib.decode_conv_la(self.k, self.hist, self.la_part, self.pos, self.base, B, self.W, self.L)
            _lib.decode_post_la(self.la_part, self.carry, self.hist, self.fb, self.x0, z, self.pos, self.base, B, self.L)
            return z
        _lib.decode_pre(x2, self.bin, self.w, self.b, self.tail, self.hist, self.x0, self.pos, self.L)
        _lib.decode_conv(self.k, self.hist, self.part, self.pos, B, self.L)
        _lib.decode_post(self.part, self.hist, self.fb, self.x0, z, self.pos, B, self.L)
        return z

    def _block_buffers(self, B, T):
        """the block step's scratch for (B, T): allocated on first use, grown when a larger block comes, never shrunk"""
        need = {"x0": B * T * self.D, "z": B * T * self.D,
                "part": int(_lib.lib().hyena_decode_block_partial_floats(B, self.D, self.L, T))}
        if self.block_buf is None or any(self.block_buf[n].numel() < need[n] for n in need):
            dev = self.hist.device
            have = {n: 0 if self.block_buf is None else self.block_buf[n].numel() for n in need}
            self.block_buf = {n: torch.empty(max(need[n], have[n]), dtype=self.dtype if n == "z" else torch.float32, device=dev) for n in need}
        buf = self.block_buf
        return buf["part"], buf["x0"][:need["x0"]].view(B, T, self.D), buf["z"][:need["z"]].view(B, T, self.D)

    def step_block(self, x3):
        """x3 (B, T, 3D), 1 <= T <= 64: in_proj output of T known positions without bias -> z (B, T, D) for out_proj; the position advances
        by T.  Three kernels that stream the history once for the T positions; the results (z, history, tail, position) equal those of T
        calls of ``step`` bit for bit.  ``z`` is a view of the cache's scratch: the next block step overwrites it."""
        if self.ragged:
            raise NotImplementedError("a decode cache in ragged mode (prefill with lengths) has no block step: one position per row and call")
        if self.W:
            raise NotImplementedError("a decode cache with lookahead has no block step (allow_append): appending known positions inside a "
                                      "window is out of scope")
        B, T, _ = x3.shape
        if not 1 <= T <= _lib.DECODE_TMAX:
            raise ValueError(f"a block step takes 1 ... {_lib.DECODE_TMAX} positions (got {T})")
        x3 = x3.contiguous()
        part, x0, z = self._block_buffers(B, T)
        if self.fan > 1:
            if B != self.B:
                raise ValueError(f"a step of a decode cache with fan = {self.fan} takes all {self.B} rows (got {B})")
            _lib.decode_pre_block_fan(x3, self.bin, self.w, self.b, self.tail, self.hist, x0, self.pos, self.L, self.S)
            _lib.decode_conv_block_fan(self.k, self.hist_shared, self.hist, part, self.pos, B, self.fan, T, self.L, self.S)
            _lib.decode_post_block_fan(part, self.hist, self.fb, x0, z, self.pos, self.fan, self.L, self.S)
            return z
        _lib.decode_pre_block(x3, self.bin, self.w, self.b, self.tail, self.hist, x0, self.pos, self.L)
        _lib.decode_conv_block(self.k, self.hist, part, self.pos, B, T, self.L)
        _lib.decode_post_block(part, self.hist, self.fb, x0, z, self.pos, self.L)
        return z

    def reorder(self, parents):
        """This package's ``_reorder_cache``: row b of the cache continues as what row ``parents[b]`` was.  ``parents``: device int32
        (B,), every entry a row of b's own fan group (an entry outside it leaves row b as it is).  In place, one kernel on the current
        stream that reads the position from device memory -- it may be captured with the step.  It moves the columns written since the
        prompt and the short filter's tail, ``2 B D (t - prompt_len)`` elements in all: the prompt's columns are the same in every row of
        a group (``hist_shared`` below S, replicated by the prefill from S on) and stay where they are, however long the prompt is.

        Fan-out caches only: the rows of a plain cache share nothing, and a caller who wants to prune, resample or branch rows builds the
        cache with ``fan=n``.  Ragged caches and caches with lookahead are refused likewise, before anything moves."""
        if self.W:
            raise NotImplementedError("reorder() on a cache with lookahead is out of scope: the carry belongs to its row's history")
        if self.ragged:
            raise NotImplementedError("reorder() on a ragged cache (prefill with lengths) is out of scope: one position per row")
        if self.fan == 1:
            raise NotImplementedError("reorder() re-parents the rows of a fan group: build the cache with fan=n (a cache with fan = 1 has "
                                      "no groups)")
        if not torch.is_tensor(parents) or parents.dtype != torch.int32 or parents.shape != (self.B,) or parents.device != self.hist.device:
            what = f"{tuple(parents.shape)} {parents.dtype} on {parents.device}" if torch.is_tensor(parents) else type(parents).__name__
            raise ValueError(f"parents must be a ({self.B},) int32 tensor on {self.hist.device} (got {what})")
        if self.fan > _lib.DECODE_BEAM_MAX:
            raise NotImplementedError(f"reorder() serves groups of at most {_lib.DECODE_BEAM_MAX} rows (this cache has fan = {self.fan})")
        _lib.decode_reorder_fan(self.hist, self.tail, parents.contiguous(), self.pos, self.B, self.fan, self.L, self.S, self.prompt_len)


class DeviceSampler:
    """The token sampler of cached generation as one kernel per step (csrc/decode_kernels.h decode_sample_kernel; semantics in
    include/hyena_decode.h): greedy / top-k / top-p with a seeded draw, EOS and padding, all of its state in device memory.

    ``seq`` (B, ncols) int64 holds the prompts and ``pad`` elsewhere; ``col`` (int32 (B,)) the column every row writes next; ``done`` which
    rows have emitted ``eos``; ``seed`` one int64.  ``sampler(logits, nxt)`` draws every row's token from ``logits`` (B, V <= 64), writes it to
    ``seq[b, col[b]]`` and to ``nxt`` (the model's next input ids, (B, 1) int64) and advances ``col`` -- nothing is read on the host, so a
    captured graph may end with the call (``GraphedDecodeStep(..., sampler=...)``)."""

    def __init__(self, seq, col, seed, temperature=1.0, top_k=1, top_p=1.0, eos=None, pad=0, vocab=None, want_scores=False, V=None, allow=None,
                 want_logprobs=False, n_new=None, automaton_tables=None):
        """``allow``: int64 bit masks, (N,) for every row or (B, N): bit v of allow[b, i] lets token v be row b's i-th new token, counted
        from ``col`` as it stands now (``token_mask``, ``iupac_constraints``).  ``want_logprobs``: ``logprobs`` (B, ``n_new``; default ncols) fp32 receives at
        [b, i] the log-probability of row b's i-th new token under the softmax of its live logits at temperature 1 (NaN where none was
        written).  Either one selects hyena_decode_sample_constrained; with neither the sampler runs hyena_decode_sample as before.
        ``automaton_tables`` = (M (Nt, S) int64, delta (S, V) int32, dstate (B,) int32) on the device, instead of ``allow``:
        hyena_decode_sample_automaton -- row b's mask is M[i, dstate[b]] and ``dstate``, which the sampler owns from here on, follows
        ``delta`` (``automaton_step_tables``; 8 Nt S + 4 S V + 4 B bytes)."""
        dev = seq.device
        self.seq, self.col = seq, col
        self.done = torch.zeros_like(col)
        self.seed = seed
        self.temperature, self.top_k, self.top_p = float(temperature), int(top_k), float(top_p)
        self.eos, self.pad, self.vocab = (-1 if eos is None else int(eos)), int(pad), vocab
        self.scores = torch.zeros(seq.shape[0], seq.shape[1], V, dtype=torch.float32, device=dev) if want_scores else None
        self.allow = allow
        self.automaton = automaton_tables
        if automaton_tables is not None and allow is not None:
            raise ValueError("a sampler with automaton_tables takes its positional masks inside M: allow must be None")
        self.dstate = None if automaton_tables is None else automaton_tables[2]
        self.start = col.clone() if allow is not None or want_logprobs or automaton_tables is not None else None
        self.logprobs = None
        if want_logprobs:
            self.logprobs = torch.full((seq.shape[0], max(int(seq.shape[1] if n_new is None else n_new), 1)), float("nan"), dtype=torch.float32,
                                       device=dev)

    def __call__(self, logits, nxt):
        _lib.decode_sample(logits, self.seed, self.col, self.done, self.seq, nxt, temperature=self.temperature, top_k=self.top_k,
                           top_p=self.top_p, eos=self.eos, pad=self.pad, vocab=self.vocab, scores=self.scores, allow=self.allow,
                           start=self.start, logprobs=self.logprobs, **({} if self.automaton is None else dict(automaton=self.automaton)))

    def snapshot(self, steps):
        """what up to ``steps`` calls from here may change -- col, done, the automaton states, the columns col[b] ... col[b] + steps - 1 of
        seq (and of scores), the slots col[b] - start[b] ... + steps - 1 of logprobs -- as a function that puts it back
        (``GraphedDecodeStep``'s warm-up steps run the real kernel)"""
        ncols = self.seq.shape[1]
        col, done = self.col.clone(), self.done.clone()
        dstate = None if self.dstate is None else self.dstate.clone()
        idx = (col.to(torch.int64)[:, None] + torch.arange(int(steps), device=col.device)).clamp_(0, ncols - 1)      # (B, steps)
        seq = self.seq.gather(1, idx)
        sidx = None if self.scores is None else idx[:, :, None].expand(-1, -1, self.scores.shape[2])
        scores = None if self.scores is None else self.scores.gather(1, sidx)
        pidx = None if self.logprobs is None else (idx - self.start.to(torch.int64)[:, None]).clamp_(0, self.logprobs.shape[1] - 1)
        logprobs = None if self.logprobs is None else self.logprobs.gather(1, pidx)

        def restore():
            self.col.copy_(col)
            self.done.copy_(done)
            if dstate is not None:
                self.dstate.copy_(dstate)
            self.seq.scatter_(1, idx, seq)
            if scores is not None:
                self.scores.scatter_(1, sidx, scores)
            if logprobs is not None:
                self.logprobs.scatter_(1, pidx, logprobs)
        return restore


class BeamSearcher:
    """Beam search over a fan-out cache as the counterpart of ``DeviceSampler``, with its call protocol: ``searcher(logits, nxt)`` runs the
    beam kernel (csrc/decode_kernels.h decode_beam_kernel; semantics in include/hyena_decode.h) on ``logits`` (G k, V <= 64) and then
    ``reorder(parent)`` on every layer's cache, all on the current stream and with nothing read on the host.
    ``GraphedDecodeStep(model, ip, G * k, sampler=searcher)`` therefore captures the model step, the beam step and the n_layer reorders
    as one graph.

    ``states``: the ``HyenaDecodeState`` of every layer, built with ``fan=k, prompt_len=P`` (``ip.key_value_memory_dict.values()``), after
    the prefill.  The k rows of group g are the beams of prompt g, best first.  State, all in device memory: ``score`` (fp32 cumulative
    log-probability, 0 / -inf before the first call so that the k identical rows expand as one), ``done``, ``col``, ``parent`` (the last
    step's parents) and the records ``tok_hist`` / ``parent_hist`` / ``lp_hist`` (G k, n_new), which ``finalize`` reads backwards."""

    def __init__(self, states, prompts, k, n_new, eos=None, pad=0, vocab=None, allow=None, automaton_tables=None):
        self.states = list(states)
        self.prompts = prompts                                   # (G, P) int64
        G, P = prompts.shape
        dev = prompts.device
        self.G, self.k, self.P, self.N = G, int(k), P, int(n_new)
        if not 1 <= self.k <= _lib.DECODE_BEAM_MAX:
            raise ValueError(f"a beam search keeps 1 ... {_lib.DECODE_BEAM_MAX} beams per prompt (got {k})")
        for s in self.states:
            if s.fan != self.k or s.B != G * self.k or getattr(s, "prompt_len", None) != P:
                raise ValueError(f"the decode caches must be built with fan = {self.k} for {G} prompts of {P} positions")
        B = G * self.k
        self.eos, self.pad, self.vocab, self.allow = (-1 if eos is None else int(eos)), int(pad), vocab, allow
        # (M, delta, dstate) as for DeviceSampler: hyena_decode_beam_automaton -- the state of a beam travels with it inside the beam kernel
        self.automaton = automaton_tables
        if automaton_tables is not None and allow is not None:
            raise ValueError("a searcher with automaton_tables takes its positional masks inside M: allow must be None")
        self.dstate = None if automaton_tables is None else automaton_tables[2]
        self.col = torch.full((B,), P, dtype=torch.int32, device=dev)
        self.start = self.col.clone()
        self.done = torch.zeros(B, dtype=torch.int32, device=dev)
        self.score = torch.full((G, self.k), float("-inf"), dtype=torch.float32, device=dev)
        self.score[:, 0] = 0.0
        self.score = self.score.reshape(B)
        self.parent = torch.arange(B, dtype=torch.int32, device=dev)
        width = max(self.N, 1)
        self.tok_hist = torch.full((B, width), self.pad, dtype=torch.int32, device=dev)
        self.parent_hist = self.parent[:, None].repeat(1, width).contiguous()
        self.lp_hist = torch.zeros(B, width, dtype=torch.float32, device=dev)
        self.calls = 0                                            # calls issued from the host (a replayed graph does not count)

    def __call__(self, logits, nxt):
        _lib.decode_beam(logits, self.score, self.col, self.done, self.start, self.parent, nxt, self.k, self.P + self.N, eos=self.eos,
                         pad=self.pad, vocab=self.vocab, allow=self.allow, tok_hist=self.tok_hist, parent_hist=self.parent_hist,
                         lp_hist=self.lp_hist, **({} if self.automaton is None else dict(automaton=self.automaton)))
        for s in self.states:
            s.reorder(self.parent)
        self.calls += 1

    def snapshot(self, steps):
        """what up to ``steps`` calls from here may change, as a function that puts it back (``GraphedDecodeStep``'s warm-up steps run the
        real kernels): the searcher's own state and, for every layer, the history columns [P, P + calls so far + steps) that the warm-up's
        reorders permute (``GraphedDecodeStep`` restores ``tail`` and ``pos`` itself, before it calls this)"""
        own = [(t, t.clone()) for t in (self.score, self.col, self.done, self.parent, self.tok_hist, self.parent_hist, self.lp_hist, self.dstate)
               if t is not None]
        calls = self.calls
        hist = []
        for s in self.states:
            lo = self.P - s.S
            hi = min(lo + calls + int(steps), s.L - s.S)
            hist.append((s.hist[:, :, lo:hi], s.hist[:, :, lo:hi].clone()))

        def restore():
            for t, saved in own + hist:
                t.copy_(saved)
            self.calls = calls
        return restore

    def finalize(self, n_done, n_return=None, want_logprobs=False):
        """after ``n_done`` calls: the ``n_return`` (default k) best beams of every prompt, best first -> ``sequences`` (G n_return, P + N)
        int64 (the prompt, the beam's tokens, ``pad`` from column P + n_done on), ``sequences_scores`` (G n_return,) fp32, and
        ``logprobs`` (G n_return, n_done) fp32 or None"""
        n = self.k if n_return is None else int(n_return)
        if not 1 <= n <= self.k:
            raise ValueError(f"n_return={n_return}: 1 ... {self.k} of the beams")
        dev = self.prompts.device
        seq = torch.full((self.G * n, self.P + self.N), self.pad, dtype=torch.int64, device=dev)
        seq[:, :self.P] = self.prompts.repeat_interleave(n, 0)
        lp = torch.zeros(self.G * n, max(int(n_done), 1), dtype=torch.float32, device=dev) if want_logprobs else None
        _lib.decode_beam_backtrack(self.tok_hist, self.parent_hist, self.lp_hist, self.k, n_done, n, seq, self.P, logprobs=lp)
        scores = self.score.view(self.G, self.k)[:, :n].reshape(-1).clone()
        return seq, scores, (None if lp is None else lp[:, :int(n_done)])


# ---- allowed-token masks for the device sampler: pure host code ----------------------------------------------------------------------------
ALL_TOKENS = -1                                     # every bit set: an unconstrained position
IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT",
         "H": "ACT", "V": "ACG", "N": "ACGT"}


def token_mask(ids):
    """the 64-bit mask with bit v set for every v in ``ids``, as the int an int64 tensor holds (bit 63 makes it negative)"""
    m = 0
    for v in ids:
        v = int(v)
        if not 0 <= v < _lib.SAMPLE_MAX_V:
            raise ValueError(f"token id {v}: a mask has one bit per logit column, 0 ... {_lib.SAMPLE_MAX_V - 1}")
        m |= 1 << v
    return m - (1 << 64) if m >> 63 else m


def iupac_constraints(pattern, token_of=None):
    """``pattern``: one character per new token, an IUPAC nucleotide code (A C G T, R Y S W K M B D H V N -- N: any of the four bases) or
    ``.`` for an unconstrained position -> (len(pattern),) int64 masks on the CPU, for ``generate(constraints=...)`` after ``.to(device)``.
    ``token_of`` maps 'A' 'C' 'G' 'T' to token ids; default: the character tokenizer's (tokenizer.DNACharTokenizerLUT)."""
    if token_of is None:
        from .tokenizer import DNACharTokenizerLUT
        token_of = DNACharTokenizerLUT().vocab
    out = []
    for i, ch in enumerate(pattern):
        if ch == ".":
            out.append(ALL_TOKENS)
        elif ch.upper() in IUPAC:
            out.append(token_mask(token_of[base] for base in IUPAC[ch.upper()]))
        else:
            raise ValueError(f"pattern[{i}] = {ch!r}: an IUPAC nucleotide code ({' '.join(IUPAC)}) or '.'")
    return torch.tensor(out, dtype=torch.int64)


# ---- token automata: constraints on what a row contains, not on where ------------------------------------------------------------------------
# Pure host code up to the tables the kernels read (hyena_decode_sample_automaton, hyena_decode_beam_automaton in include/hyena_decode.h).
IUPAC_COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A", "R": "Y", "Y": "R", "S": "S", "W": "W", "K": "M", "M": "K", "B": "V", "V": "B",
                    "D": "H", "H": "D", "N": "N"}


class TokenAutomaton:
    """A deterministic automaton over the token alphabet, for ``generate(automaton=...)``: every returned row spells a word it accepts.

    ``delta`` (S, V) int32: ``delta[s, v]`` is the state after token v in state s, -1 where v is forbidden there; V is the number of logit
    columns (at most 64), 1 <= S <= 4096.  ``accept`` (S,) bool: the states a finished row may stand in (default: all).  ``start``: the state
    before the first token.  ``context``: how many trailing prompt tokens the automaton reads, from ``start``, before the first new token
    (a forbidden transition inside the prompt restarts it from ``start``).  The tensors are kept on the CPU."""

    def __init__(self, delta, accept=None, start=0, context=0):
        if not torch.is_tensor(delta) or delta.dim() != 2 or delta.dtype != torch.int32:
            what = f"{tuple(delta.shape)} {delta.dtype}" if torch.is_tensor(delta) else type(delta).__name__
            raise ValueError(f"delta must be an (S, V) int32 tensor (got {what})")
        S, V = delta.shape
        if not 1 <= S <= _lib.AUTOMATON_MAX_STATES:
            raise ValueError(f"an automaton has 1 ... {_lib.AUTOMATON_MAX_STATES} states (delta has {S} rows)")
        if not 1 <= V <= _lib.SAMPLE_MAX_V:
            raise ValueError(f"an automaton reads 1 ... {_lib.SAMPLE_MAX_V} tokens, one per logit column (delta has {V} columns)")
        delta = delta.detach().cpu().contiguous()
        if int(delta.min()) < -1 or int(delta.max()) >= S:
            raise ValueError(f"delta holds states in [0, {S}) and -1 for a forbidden token (got {int(delta.min())} ... {int(delta.max())})")
        if accept is None:
            accept = torch.ones(S, dtype=torch.bool)
        if not torch.is_tensor(accept) or accept.shape != (S,) or accept.dtype != torch.bool:
            what = f"{tuple(accept.shape)} {accept.dtype}" if torch.is_tensor(accept) else type(accept).__name__
            raise ValueError(f"accept must be a ({S},) bool tensor (got {what})")
        if not 0 <= int(start) < S:
            raise ValueError(f"start={start}: a state in [0, {S})")
        if int(context) < 0:
            raise ValueError(f"context={context}: a number of prompt tokens")
        self.delta, self.accept, self.start, self.context = delta, accept.detach().cpu().contiguous(), int(start), int(context)
        self.S, self.V = S, V

    def walk(self, tokens, state=None):
        """the states after every token of ``tokens`` from ``state`` (default ``start``) -> list of ints; -1 from a forbidden token on"""
        s = self.start if state is None else int(state)
        out = []
        for v in tokens:
            v = int(v)
            s = int(self.delta[s, v]) if s >= 0 and 0 <= v < self.V else -1
            out.append(s)
        return out

    def accepts(self, tokens, state=None):
        """no forbidden transition on the way and an accepting state at the end"""
        s = ([self.start if state is None else int(state)] + self.walk(tokens, state))[-1]
        return s >= 0 and bool(self.accept[s])

    def initial_state(self, prompt):
        """the state before the first new token: the automaton run from ``start`` over the last ``min(context, len(prompt))`` tokens of
        ``prompt``; a forbidden transition on the way restarts it from ``start``"""
        s = self.start
        tail = list(prompt)[len(prompt) - min(self.context, len(prompt)):]
        for v in tail:
            v = int(v)
            t = int(self.delta[s, v]) if 0 <= v < self.V else -1
            s = self.start if t < 0 else t
        return s


def motif_automaton(avoid=(), require=(), max_homopolymer=None, reverse_complement=False, token_of=None, n_tokens=16):
    """The automaton of a DNA designer's content constraints -> ``TokenAutomaton`` over ``n_tokens`` tokens.

    ``avoid`` / ``require``: IUPAC strings (``IUPAC``; ``token_of`` as for ``iupac_constraints``).  No transition may complete an occurrence of
    an avoided motif; every required motif must occur (one "seen" bit per listed motif; ``accept``: all seen).  ``reverse_complement=True``
    adds the reverse complement of every motif: an avoided motif is avoided on both strands, a required one counts on either.
    ``max_homopolymer=h``: no run of h + 1 equal bases.  A token that is not one of the four bases breaks every motif and every run (it keeps
    the seen bits).  Built by subset construction over sets of (motif, prefix length), so an IUPAC class costs no expansion; not minimised.
    ``context`` = the longest motif - 1, or h if that is larger.  More than 4096 states: ValueError."""
    if token_of is None:
        from .tokenizer import DNACharTokenizerLUT
        token_of = DNACharTokenizerLUT().vocab
    V = int(n_tokens)
    if not 1 <= V <= _lib.SAMPLE_MAX_V:
        raise ValueError(f"n_tokens={n_tokens}: 1 ... {_lib.SAMPLE_MAX_V} logit columns")
    bases = "ACGT"
    ids = [int(token_of[b]) for b in bases]
    if len(set(ids)) != 4 or not all(0 <= v < V for v in ids):
        raise ValueError(f"token_of maps A C G T to {ids}: four different ids below n_tokens = {V}")
    h = None if max_homopolymer is None else int(max_homopolymer)
    if h is not None and h < 1:
        raise ValueError(f"max_homopolymer={max_homopolymer}: at least 1")

    def classes(motif, what):
        motif = str(motif).upper()
        if not motif or any(ch not in IUPAC for ch in motif):
            raise ValueError(f"{what} motif {motif!r}: a non-empty string of IUPAC nucleotide codes ({' '.join(IUPAC)})")
        out = [motif]
        if reverse_complement:
            rc = "".join(IUPAC_COMPLEMENT[ch] for ch in reversed(motif))
            if rc != motif:
                out.append(rc)
        return [[frozenset(bases.index(b) for b in IUPAC[ch]) for ch in m] for m in out]

    motifs = []                                                  # (classes per position, seen bit or None for an avoided motif)
    for m in avoid:
        motifs += [(c, None) for c in classes(m, "avoid")]
    n_req = 0
    for m in require:
        motifs += [(c, n_req) for c in classes(m, "require")]
        n_req += 1
    all_seen = (1 << n_req) - 1
    limit = _lib.AUTOMATON_MAX_STATES

    def step(state, b):
        """state (partial matches, last base, run, seen) after base b (0 .. 3) -> state, or None: forbidden"""
        part, last, run, seen = state
        if h is not None:
            run = run + 1 if b == last else 1
            last = b
            if run > h:
                return None
        nxt = set()
        for mi, p in list(part) + [(mi, 0) for mi in range(len(motifs))]:
            cls, bit = motifs[mi]
            if b in cls[p]:
                if p + 1 == len(cls):
                    if bit is None:
                        return None
                    seen |= 1 << bit
                else:
                    nxt.add((mi, p + 1))
        return (frozenset(nxt), last, run, seen)

    first = (frozenset(), -1, 0, 0)
    index, order, rows = {first: 0}, [first], []
    while len(rows) < len(order):
        state = order[len(rows)]
        row = []
        for b in range(4):
            t = step(state, b)
            if t is not None and t not in index:
                if len(order) >= limit:
                    raise ValueError(f"these motifs need more than {limit} automaton states (the limit of a token automaton)")
                index[t] = len(order)
                order.append(t)
            row.append(-1 if t is None else index[t])
        t = (frozenset(), -1, 0, state[3])                      # any other token: no prefix, no run, the seen bits kept
        if t not in index:
            if len(order) >= limit:
                raise ValueError(f"these motifs need more than {limit} automaton states (the limit of a token automaton)")
            index[t] = len(order)
            order.append(t)
        row.append(index[t])
        rows.append(row)
    S = len(order)
    delta = torch.empty(S, V, dtype=torch.int32)
    table = torch.tensor(rows, dtype=torch.int32)               # (S, 5): A C G T, other
    delta[:] = table[:, 4:5]
    for b, v in enumerate(ids):
        delta[:, v] = table[:, b]
    accept = torch.tensor([st[3] == all_seen for st in order], dtype=torch.bool)
    longest = max([len(c) for c, _ in motifs], default=1)
    return TokenAutomaton(delta, accept, start=0, context=max(longest - 1, h or 0))


def _mask_ints(bits):
    """bool (..., V <= 64) -> int64 (...) with bit v set where bits[..., v] (bit 63 is the sign)"""
    V = bits.shape[-1]
    w = torch.tensor([(1 << v) - (1 << 64 if v == 63 else 0) for v in range(V)], dtype=torch.int64)
    return (bits.to(torch.int64) * w).sum(-1)


def automaton_step_tables(automaton, N, masks=None, eos=None, vocab=None, positional=None):
    """The step table of N new tokens -> ``M`` (Nt, S) int64 on the CPU: bit v of M[i, s] says that token v may be the i-th new token in
    state s, i.e. that an accepted word can still be completed after it.  Backwards from the end:
        live[N][s] = accept[s]
        M[i][s]    = { v != eos : v in P_i, delta[s, v] >= 0, live[i + 1][delta[s, v]] }  u  { eos : eos in P_i, accept[s] }
        live[i][s] = M[i][s] is not empty
    ``masks``: the positional sets P_i as (N,) int64 bit masks (None: every token), already without eos where ``min_new_tokens`` holds it
    back; ``vocab``: only tokens below it.  ``positional`` says whether anything depends on i (default: masks given, or an automaton with
    a rejecting state); where nothing does, Nt = 1 and M[0] is the greatest fixed point of the recursion -- only transitions into states
    without an infinite continuation are pruned, and one row serves a generation of any length.  Otherwise Nt = N, N S <= 2^22."""
    A, N = automaton, int(N)
    S, V = A.S, A.V
    Vlive = V if vocab is None else int(vocab)
    e = None if eos is None or not 0 <= int(eos) < V else int(eos)
    ok = A.delta >= 0                                            # (S, V)
    to = A.delta.clamp(min=0).to(torch.int64)
    ok[:, Vlive:] = False
    if e is not None:
        ok[:, e] = False
    cols = torch.arange(V)
    if masks is None:
        P = torch.ones(max(N, 1), V, dtype=torch.bool)
    else:
        P = ((masks.detach().cpu().to(torch.int64)[:, None] >> cols[None]) & 1).bool()      # (N, V)
    if positional is None:
        positional = masks is not None or not bool(A.accept.all())
    ends = torch.zeros(S, V, dtype=torch.bool)                   # eos, where the state accepts
    if e is not None and e < Vlive:
        ends[:, e] = A.accept
    if not positional:
        live = torch.ones(S, dtype=torch.bool)
        while True:
            bits = ((ok & live[to]) | ends) & P[0][None]
            new = bits.any(1)
            if bool((new == live).all()):
                return _mask_ints(bits)[None].contiguous()
            live = new
    if N * S > _lib.AUTOMATON_MAX_TABLE:
        raise ValueError(f"an automaton of {S} states over {N} new tokens needs a step table of {N * S} entries: the limit is "
                         f"{_lib.AUTOMATON_MAX_TABLE} (2^22)")
    M = torch.zeros(max(N, 1), S, dtype=torch.int64)
    live = A.accept.clone()
    for i in range(N - 1, -1, -1):
        bits = ((ok & live[to]) | ends) & P[i][None]
        M[i] = _mask_ints(bits)
        live = bits.any(1)
    return M
