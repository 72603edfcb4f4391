"""Block decode step -- T known positions appended to a live cache in one pass (csrc/decode_kernels.h decode_*_block,
HyenaDecodeState.step_block, HyenaOperator.forward at seqlen_offset > 0 with several positions, HyenaDNALM.score_continuations) -- under
tests/hipemu: the block kernels bit for bit against T calls of the single-position kernels (plain and fan-out layout, three dtypes), the
out-of-range and argument refusals, the cache's scratch, the language model's appended logits against the full forward."""
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SOURCES = [os.path.join(ROOT, "hyena_dna_amd", "csrc", "decode_kernels.h"), os.path.join(ROOT, "hyena_dna_amd", "csrc", "cm.hip"),
               os.path.join(ROOT, "include", "hyena_decode.h")]
CHUNK = 8192
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# (Lcap, t0, T): taps before position 0 | one position | one tile | tile remainder | across the chunk and a vector boundary | a chunk's
# first position | ends exactly at Lcap | the longest block, third chunk
PLAIN_CASES = [(8300, 0, 4), (8300, 1, 3), (8300, 100, 1), (8300, 100, 16), (8300, 100, 17), (8300, 8185, 16), (8300, 8192, 5), (8300, 8284, 16),
               (16500, 16389, 64)]
# (Lcap, P, t0, T): the cases above from position 1 on for prompts of P in {1, 100, 8192, 8200, 16389}: S = 0, 0, 8192, 8192, 16384
FAN_CASES = [(8300, 1, 1, 3), (8300, 100, 100, 1), (8300, 100, 100, 16), (8300, 100, 100, 17), (8300, 100, 8185, 16), (8300, 8192, 8192, 5),
             (8300, 8200, 8284, 16), (16500, 16389, 16389, 64), (16500, 8200, 16389, 64)]


@pytest.fixture()
def decode_emu(emu_backend):
    """the emulation library of emu_backend, rebuilt if the decode kernels are newer than it (build_emu's freshness check does not list them)"""
    from tests.hipemu import build_emu
    if not os.path.exists(build_emu.OUT) or any(os.path.getmtime(f) > os.path.getmtime(build_emu.OUT) for f in NEW_SOURCES):
        build_emu.build(force=True)
        emu_backend._lib = None
    return emu_backend


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


class BlockCase:
    """A cache state at position t0 -- B = G n rows; fan: the layout of a prompt of P positions (columns below S = P // 8192 * 8192 once per
    group) -- twice: ``one`` is advanced by the single-position kernels, ``blk`` by the block kernels.  Shared by the device tests
    (tests/test_gpu_decode_block.py)."""

    def __init__(self, _lib, D, G, n, Lcap, t0, dtype, fan=False, P=None, dev="cpu", seed=0):
        g = torch.Generator(device=dev).manual_seed(seed)
        B = G * n
        S = P // CHUNK * CHUNK if fan else 0
        self.lib, self.D, self.G, self.n, self.B, self.Lcap, self.S, self.dtype, self.dev, self.g, self.fan = _lib, D, G, n, B, Lcap, S, dtype, dev, g, fan
        ldk = _lib.row_pitch(Lcap)
        self.k = (torch.randn(D, ldk, generator=g, device=dev) * torch.exp(-3.0 * torch.linspace(0, 1, ldk, device=dev))[None])[:, :Lcap]
        self.fb = torch.randn(D, generator=g, device=dev)
        self.w = torch.randn(3 * D, 3, generator=g, device=dev) * 0.5
        self.b = torch.randn(3 * D, generator=g, device=dev) * 0.2
        self.bin = torch.randn(3 * D, generator=g, device=dev) * 0.3
        hist = torch.randn(B, D, t0, generator=g, device=dev).to(dtype)
        if S > 0:
            hist[:, :, :S] = hist[::n, :, :S].repeat_interleave(n, 0)
        self.shared = None
        if S > 0:
            self.shared = torch.zeros(G, D, _lib.row_pitch(S), dtype=dtype, device=dev)
            self.shared[:, :, :S] = hist[::n, :, :S]
        rows = torch.zeros(B, D, _lib.row_pitch(max(Lcap - S, 1)), dtype=dtype, device=dev)
        rows[:, :, :t0 - S] = hist[:, :, S:]
        tail = torch.randn(3 * D, B, 2, generator=g, device=dev).to(dtype).float()
        pos = torch.tensor([t0], dtype=torch.int32, device=dev)
        self.shared0 = None if self.shared is None else self.shared.clone()
        self.one = dict(rows=rows, tail=tail, pos=pos)
        self.blk = dict(rows=rows.clone(), tail=tail.clone(), pos=pos.clone())
        self.part_one = _lib.decode_partials(B, D, Lcap, dev)

    def new_x(self, T):
        return torch.randn(self.B, T, 3 * self.D, generator=self.g, device=self.dev).to(self.dtype)

    def step_one(self, x2):
        _lib, s = self.lib, self.one
        x0, z = torch.empty(self.B, self.D, device=self.dev), torch.empty(self.B, self.D, dtype=self.dtype, device=self.dev)
        self.part_one.fill_(float("nan"))                       # a slot that was not written in this step must never be read
        if self.fan:
            _lib.decode_pre_fan(x2, self.bin, self.w, self.b, s["tail"], s["rows"], x0, s["pos"], self.Lcap, self.S)
            _lib.decode_conv_fan(self.k, self.shared, s["rows"], self.part_one, s["pos"], self.B, self.n, self.Lcap, self.S)
            _lib.decode_post_fan(self.part_one, s["rows"], self.fb, x0, z, s["pos"], self.B, self.n, self.Lcap, self.S)
        else:
            _lib.decode_pre(x2, self.bin, self.w, self.b, s["tail"], s["rows"], x0, s["pos"], self.Lcap)
            _lib.decode_conv(self.k, s["rows"], self.part_one, s["pos"], self.B, self.Lcap)
            _lib.decode_post(self.part_one, s["rows"], self.fb, x0, z, s["pos"], self.B, self.Lcap)
        return z, x0

    def step_block(self, x3, state=None):
        _lib, s = self.lib, self.blk if state is None else state
        B, T, D = self.B, x3.shape[1], self.D
        x0 = torch.full((B, T, D), float("nan"), device=self.dev)
        z = torch.full((B, T, D), float("nan"), dtype=self.dtype, device=self.dev)
        part = _lib.decode_block_partials(B, D, self.Lcap, T, self.dev).fill_(float("nan"))
        if self.fan:
            _lib.decode_pre_block_fan(x3, self.bin, self.w, self.b, s["tail"], s["rows"], x0, s["pos"], self.Lcap, self.S)
            _lib.decode_conv_block_fan(self.k, self.shared, s["rows"], part, s["pos"], B, self.n, T, self.Lcap, self.S)
            _lib.decode_post_block_fan(part, s["rows"], self.fb, x0, z, s["pos"], self.n, self.Lcap, self.S)
        else:
            _lib.decode_pre_block(x3, self.bin, self.w, self.b, s["tail"], s["rows"], x0, s["pos"], self.Lcap)
            _lib.decode_conv_block(self.k, s["rows"], part, s["pos"], B, T, self.Lcap)
            _lib.decode_post_block(part, s["rows"], self.fb, x0, z, s["pos"], self.Lcap)
        return z, x0

    def assert_same_state(self):
        assert torch.equal(self.one["rows"], self.blk["rows"])
        assert torch.equal(self.one["tail"], self.blk["tail"])
        assert torch.equal(self.one["pos"], self.blk["pos"])
        if self.shared is not None:
            assert torch.equal(self.shared, self.shared0)      # the shared history is never written

    def assert_block_bitwise(self, T):
        """one block step of T against T single steps: z, x0, history, tail, pos"""
        t0 = self.blk["pos"].item()
        before = self.blk["rows"].clone()
        x3 = self.new_x(T)
        singles = [self.step_one(x3[:, i].contiguous()) for i in range(T)]
        z, x0 = self.step_block(x3)
        assert not torch.isnan(z.float()).any() and not torch.isnan(x0).any()
        for i, (z1, g1) in enumerate(singles):
            assert torch.equal(z[:, i], z1), (t0, i)
            assert torch.equal(x0[:, i], g1), (t0, i)
        assert self.blk["pos"].item() == t0 + T
        self.assert_same_state()
        c0 = t0 - self.S                                        # nothing but the T new columns of the history changed
        assert torch.equal(self.blk["rows"][:, :, :c0], before[:, :, :c0]) and torch.equal(self.blk["rows"][:, :, c0 + T:], before[:, :, c0 + T:])


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Lcap,t0,T", PLAIN_CASES)
def test_block_kernels_equal_single_steps(decode_emu, dtype, Lcap, t0, T):
    c = BlockCase(decode_emu, D=3, G=2, n=1, Lcap=Lcap, t0=t0, dtype=dtype, seed=Lcap + t0 + T)
    c.assert_block_bitwise(T)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Lcap,P,t0,T", FAN_CASES)
def test_block_fan_kernels_equal_single_fan_steps(decode_emu, dtype, Lcap, P, t0, T):
    c = BlockCase(decode_emu, D=3, G=2, n=3, Lcap=Lcap, t0=t0, dtype=dtype, fan=True, P=P, seed=Lcap + P + t0 + T)
    assert c.S == {1: 0, 100: 0, 8192: 8192, 8200: 8192, 16389: 16384}[P]
    c.assert_block_bitwise(T)


@pytest.mark.parametrize("fan", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_block_and_single_steps_interleave(decode_emu, dtype, fan):
    """single, block(5), single, block(16) on one cache against the same 23 positions as single steps on the other, across the chunk boundary"""
    c = BlockCase(decode_emu, D=3, G=2, n=3 if fan else 1, Lcap=8300, t0=8180, dtype=dtype, fan=fan, P=100, seed=11)
    got, ref = [], []
    for T in (1, 5, 1, 16):
        x3 = c.new_x(T)
        ref += [c.step_one(x3[:, i].contiguous()) for i in range(T)]
        if T == 1:                                             # a single-position step on the block cache's state
            c.one, c.blk = c.blk, c.one
            got.append(c.step_one(x3[:, 0].contiguous()))
            c.one, c.blk = c.blk, c.one
        else:
            z, x0 = c.step_block(x3)
            got += [(z[:, i], x0[:, i]) for i in range(T)]
        c.assert_same_state()
    assert len(ref) == 23 and c.blk["pos"].item() == 8203
    for i, ((z, x0), (z1, g1)) in enumerate(zip(got, ref)):
        assert torch.equal(z, z1) and torch.equal(x0, g1), i


@pytest.mark.parametrize("fan", [False, True])
def test_block_out_of_range_does_nothing(decode_emu, fan):
    c = BlockCase(decode_emu, D=3, G=2, n=3 if fan else 1, Lcap=8300, t0=8290, dtype=torch.float32, fan=fan, P=8200, seed=3)
    for t0, T in ((8290, 11), (-1, 4)) + (((8191, 4),) if fan else ()):       # t0 + T = Lcap + 1 | a parked position | fan: below S
        c.blk["pos"].fill_(t0)
        rows, tail = c.blk["rows"].clone(), c.blk["tail"].clone()
        z, x0 = c.step_block(c.new_x(T))
        assert torch.isnan(z).all() and torch.isnan(x0).all()                   # nothing written
        assert torch.equal(c.blk["rows"], rows) and torch.equal(c.blk["tail"], tail) and c.blk["pos"].item() == t0
    c.blk["pos"].fill_(8290)
    c.one["pos"].fill_(8290)
    c.assert_block_bitwise(10)                                                   # t0 + T = Lcap: the last block that fits


def test_block_c_abi_refuses_bad_arguments(decode_emu):
    _lib = decode_emu
    L = _lib.lib()
    D, B, fan, Lcap, S, T = 2, 4, 2, 8300, 8192, 4
    k = torch.zeros(D, _lib.row_pitch(Lcap))
    h = torch.zeros(B, D, _lib.row_pitch(Lcap))
    hs, hr = torch.zeros(B // fan, D, _lib.row_pitch(S)), torch.zeros(B, D, _lib.row_pitch(Lcap - S))
    part, pos = _lib.decode_block_partials(B, D, Lcap, 64, "cpu"), torch.tensor([-1], dtype=torch.int32)       # (a parked position: a good call does nothing)
    x, w, b, tail = torch.zeros(B, 64, 3 * D), torch.zeros(3 * D, 3), torch.zeros(3 * D), torch.zeros(3 * D, B, 2)
    x0, z = torch.zeros(B, 64, D), torch.zeros(B, 64, D)
    p = lambda t: None if t is None else t.data_ptr()

    def pre(T=T, B=B, Lcap=Lcap, lda=h.stride(1), hp=p(h), xp=p(x), ldx=3 * D, posp=p(pos)):
        return L.hyena_decode_pre_block(xp, ldx, None, p(w), p(b), p(tail), hp, p(x0), posp, B, B, D, Lcap, lda, T, 0, None)

    def conv(T=T, B=B, Lcap=Lcap, lda=h.stride(1), hp=p(h), kp=p(k), ldk=k.stride(0), partp=p(part), dtype=0):
        return L.hyena_decode_conv_block(kp, ldk, hp, partp, p(pos), B, D, Lcap, lda, T, dtype, None)

    def post(T=T, B=B, Lcap=Lcap, lda=h.stride(1), hp=p(h), zp=p(z)):
        return L.hyena_decode_post_block(p(part), hp, None, p(x0), zp, p(pos), B, D, Lcap, lda, T, 0, None)

    def pre_f(T=T, S=S, ldr=hr.stride(1), hp=p(hr)):
        return L.hyena_decode_pre_block_fan(p(x), 3 * D, None, p(w), p(b), p(tail), hp, p(x0), p(pos), B, B, D, Lcap, S, ldr, T, 0, None)

    def conv_f(T=T, B=B, fan=fan, S=S, lds=hs.stride(1), ldr=hr.stride(1), hsp=p(hs), hrp=p(hr)):
        return L.hyena_decode_conv_block_fan(p(k), k.stride(0), hsp, hrp, p(part), p(pos), B, fan, D, Lcap, S, lds, ldr, T, 0, None)

    def post_f(T=T, B=B, fan=fan, S=S, ldr=hr.stride(1)):
        return L.hyena_decode_post_block_fan(p(part), p(hr), None, p(x0), p(z), p(pos), B, fan, D, Lcap, S, ldr, T, 0, None)

    calls = (pre, conv, post, pre_f, conv_f, post_f)
    assert all(f() == 0 for f in calls) and all(f(T=1) == 0 for f in calls) and all(f(T=64) == 0 for f in calls) and pos.item() == -1
    for bad in (0, 65, -1):
        assert all(f(T=bad) == 1 for f in calls), bad                                        # T outside [1, HYENA_DECODE_TMAX]
    assert L.hyena_decode_block_partial_floats(B, D, Lcap, 0) == 0 and L.hyena_decode_block_partial_floats(B, D, Lcap, 65) == 0
    assert L.hyena_decode_block_partial_floats(B, D, Lcap, 5) == 2 * B * 5 * D
    # the refusals of the single-position entry points
    assert pre(hp=p(h) + 4) == 1 and conv(hp=p(h) + 4) == 1 and post(hp=p(h) + 4) == 1         # a misaligned history
    assert pre(lda=h.stride(1) + 4) == 1 and conv(lda=h.stride(1) + 4) == 1 and post(lda=Lcap - 4) == 1
    assert conv(kp=p(k) + 4) == 1 and conv(ldk=k.stride(0) + 2) == 1 and conv(ldk=Lcap - 4) == 1
    assert pre(xp=None) == 1 and pre(posp=None) == 1 and pre(hp=None) == 1 and conv(kp=None) == 1 and conv(partp=None) == 1 and post(zp=None) == 1
    assert pre(ldx=3 * D - 1) == 1 and pre(B=0) == 1 and conv(dtype=7) == 1 and conv(Lcap=(1 << 20) + 1) == 1
    # ... and of the fan entry points
    assert conv_f(S=100) == 1 and pre_f(S=100) == 1 and post_f(S=100) == 1                  # S not a multiple of 8192
    assert conv_f(B=5) == 1 and post_f(B=5) == 1 and conv_f(fan=0) == 1 and post_f(fan=0) == 1
    assert conv_f(S=16384) == 1 and pre_f(S=16384) == 1 and post_f(S=16384) == 1            # S > Lcap
    assert conv_f(lds=S + 4) == 1 and conv_f(ldr=hr.stride(1) + 4) == 1 and pre_f(ldr=hr.stride(1) + 4) == 1 and post_f(ldr=12) == 1
    assert conv_f(hsp=p(hs) + 4) == 1 and conv_f(hrp=p(hr) + 4) == 1 and conv_f(hsp=None) == 1 and pre_f(hp=p(hr) + 4) == 1
    assert pos.item() == -1


# ---- the cache --------------------------------------------------------------------------------------------------------------------------
def _layer(l_max, **kw):
    d = dict(l_max=l_max, order=2, filter_order=64, emb_dim=5, short_filter_order=3, modulate=True, w=10, lr=6e-4, wd=0.0, lr_pos_emb=0.0)
    d.update(kw)
    return d


def _lm(L, d=64, n_layer=2, seed=0):
    from hyena_dna_amd.lm import HyenaDNALM
    torch.manual_seed(seed)
    m = HyenaDNALM(d_model=d, n_layer=n_layer, d_inner=4 * d, vocab_size=12, layer=_layer(L + 2), resid_dropout=0.0, embed_dropout=0.1,
                   pad_vocab_size_multiple=8, fused_dropout_add_ln=True, residual_in_fp32=True)
    return m.eval()


def test_step_block_equals_steps_and_reuses_its_buffers(decode_emu):
    from hyena_dna_amd.hyena import HyenaOperator
    from hyena_dna_amd.inference import InferenceParams
    torch.manual_seed(0)
    D, B, P, L = 8, 2, 10, 64
    op = HyenaOperator(d_model=D, **_layer(L)).eval()
    u = torch.randn(B, P, D)
    states = []
    with torch.no_grad():
        for _ in range(2):
            ip = InferenceParams(max_seqlen=L, max_batch_size=B, allow_append=True)
            st = ip.key_value_memory_dict[op._decode_key()] = op.allocate_inference_cache(B, L)
            op(u, inference_params=ip)
            states.append(st)
    one, blk = states
    assert blk.block_buf is None                                                # nothing until the first block step
    g = torch.Generator().manual_seed(1)
    ptrs = None
    for T, grows in ((5, True), (3, False), (16, True), (16, False), (1, False)):
        x3 = torch.randn(B, T, 3 * D, generator=g)
        z = blk.step_block(x3)
        assert z.shape == (B, T, D)
        for i in range(T):
            assert torch.equal(one.step(x3[:, i].contiguous()), z[:, i])
        assert torch.equal(one.hist, blk.hist) and torch.equal(one.tail, blk.tail) and torch.equal(one.pos, blk.pos)
        now = {n: (t.data_ptr(), t.numel()) for n, t in blk.block_buf.items()}
        if ptrs is not None:
            assert (now != ptrs) == grows, T                                     # grown for a larger block, else the same tensors
            assert all(now[n][1] >= ptrs[n][1] for n in now)                      # never shrunk
        ptrs = now
    with pytest.raises(ValueError, match="1 ... 64"):
        blk.step_block(torch.randn(B, 65, 3 * D))
    assert blk.pos.item() == P + 41


def test_step_block_refuses_a_ragged_cache(decode_emu):
    from hyena_dna_amd.hyena import HyenaOperator
    from hyena_dna_amd.inference import InferenceParams
    torch.manual_seed(0)
    D, B, P, L = 8, 2, 10, 32
    op = HyenaOperator(d_model=D, **_layer(L)).eval()
    ip = InferenceParams(max_seqlen=L, max_batch_size=B, lengths_per_sample=torch.tensor([10, 7], dtype=torch.int32), allow_append=True)
    st = ip.key_value_memory_dict[op._decode_key()] = op.allocate_inference_cache(B, L)
    with torch.no_grad():
        op(torch.randn(B, P, D), inference_params=ip)
        assert st.ragged
        with pytest.raises(NotImplementedError, match="ragged"):
            st.step_block(torch.randn(B, 4, 3 * D))
        ip.seqlen_offset = P
        with pytest.raises(NotImplementedError, match="ragged"):
            op(torch.randn(B, 4, D), inference_params=ip)


def test_operator_refuses_a_block_past_the_cache(decode_emu):
    from hyena_dna_amd.hyena import HyenaOperator
    from hyena_dna_amd.inference import InferenceParams
    torch.manual_seed(0)
    op = HyenaOperator(d_model=8, **_layer(64)).eval()
    ip = InferenceParams(max_seqlen=16, max_batch_size=2, allow_append=True)
    st = ip.key_value_memory_dict[op._decode_key()] = op.allocate_inference_cache(2, 16)
    u = torch.randn(2, 8, 8)
    with torch.no_grad():
        op(u, inference_params=ip)
        ip.seqlen_offset = 8
        with pytest.raises(ValueError, match=r"offset 8 \+ 9 positions") as e:
            op(torch.randn(2, 9, 8), inference_params=ip)
        assert "16" in str(e.value) and st.pos.item() == 8                       # refused up front: the cache has not moved
        ip.allow_append = False                                                  # without the opt-in: the refusal of before, nothing moves
        with pytest.raises(ValueError, match="one position.*allow_append"):
            op(u, inference_params=ip)
        assert st.pos.item() == 8
        ip.allow_append = True
        assert op(u, inference_params=ip).shape == (2, 8, 8) and st.pos.item() == 16


# ---- the language model ---------------------------------------------------------------------------------------------------------------------
def _prefill(m, ids, P, L):
    from hyena_dna_amd.inference import InferenceParams
    B = ids.shape[0]
    ip = InferenceParams(max_seqlen=L, max_batch_size=B, allow_append=True)
    ip.key_value_memory_dict = m.allocate_inference_cache(B, L)
    first = m(ids[:, :P], inference_params=ip)[0].logits
    ip.seqlen_offset = P
    return ip, first


def _assert_logits(got, ref, what):
    """the project's fp32 bound of tests/test_gpu_decode.py, per row and position"""
    for r in range(ref.shape[0]):
        for i in range(ref.shape[1]):
            assert _rel(got[r, i], ref[r, i]) < 1e-5, (what, r, i, _rel(got[r, i], ref[r, i]))


@pytest.mark.parametrize("P,T", [(40, 9), (5, 70)])
def test_lm_appended_block_matches_full_forward(decode_emu, P, T):
    """forward(ids[:, P:P + T]) at offset P against the plain forward over all P + T tokens; T = 70: two tiles (64 + 6)"""
    B, L = 2, P + T
    m = _lm(L)
    ids = torch.randint(7, 11, (B, L), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        ref = m(ids)[0].logits
        ip, first = _prefill(m, ids, P, L)
        got = m(ids[:, P:], inference_params=ip)[0].logits
    assert got.shape == (B, T, ref.shape[-1])
    _assert_logits(first, ref[:, :P], "prefill")
    _assert_logits(got, ref[:, P:], "block")
    for st in ip.key_value_memory_dict.values():
        assert st.pos.item() == L


def test_lm_block_then_single_steps_match_full_forward(decode_emu):
    B, P, T, N = 2, 30, 12, 4
    L = P + T + N
    m = _lm(L)
    ids = torch.randint(7, 11, (B, L), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        ref = m(ids)[0].logits
        ip, _ = _prefill(m, ids, P, L)
        outs = [m(ids[:, P:P + T], inference_params=ip)[0].logits]
        for i in range(P + T, L):
            ip.seqlen_offset = i
            outs.append(m(ids[:, i:i + 1], inference_params=ip)[0].logits)
    _assert_logits(torch.cat(outs, dim=1), ref[:, P:], "block + steps")


@pytest.mark.parametrize("G,n,P,T,vocab", [(2, 3, 20, 5, None), (2, 1, 20, 5, None), (1, 3, 12, 1, None), (2, 3, 20, 5, 12), (1, 2, 8200, 3, None)])
def test_score_continuations_matches_full_forwards(decode_emu, G, n, P, T, vocab):
    m = _lm(P + T, n_layer=1 if P > 8000 else 2)
    gen = torch.Generator().manual_seed(9)
    ctx = torch.randint(7, 11, (G, P), generator=gen)
    cont = torch.randint(7, 11, (G, n, T), generator=gen)
    lp, logits = m.score_continuations(ctx, cont, vocab_size=vocab, return_logits=True)
    assert lp.shape == (G, n, T) and lp.dtype == torch.float32 and logits.shape[:3] == (G, n, T) and logits.dtype == torch.float32
    only = m.score_continuations(ctx, cont, vocab_size=vocab)
    assert torch.equal(only, lp)
    V = logits.shape[-1] if vocab is None else vocab
    assert logits.shape[-1] == 16                                                # 12 padded to a multiple of 8
    assert torch.equal(lp, torch.log_softmax(logits[..., :V], dim=-1).gather(-1, cont.unsqueeze(-1)).squeeze(-1))
    with torch.no_grad():
        for g in range(G):
            for j in range(n):
                ref = m(torch.cat([ctx[g], cont[g, j]])[None])[0].logits[:, P - 1:P + T - 1].float()
                _assert_logits(logits[g, j][None], ref, ("score", g, j))
    if vocab is not None:                                                        # the padded columns take no mass
        assert not torch.equal(lp, m.score_continuations(ctx, cont))
    assert (lp <= 0).all()


def test_score_continuations_refusals(decode_emu):
    m = _lm(30)
    ctx = torch.randint(7, 11, (2, 20))
    cont = torch.randint(7, 11, (2, 3, 5))
    cont[0, 0, 0] = 10
    with pytest.raises(ValueError, match=r"\(G, P\)"):
        m.score_continuations(ctx[0], cont)
    with pytest.raises(ValueError, match=r"\(G, n, T\)"):
        m.score_continuations(ctx, cont[:, 0])
    with pytest.raises(ValueError, match=r"\(G, n, T\)"):
        m.score_continuations(ctx, cont[:1])                                     # another number of contexts
    with pytest.raises(ValueError, match="at least one"):
        m.score_continuations(ctx, cont[:, :, :0])
    with pytest.raises(ValueError, match=r"20\) \+ continuation \(14\) - 1 = 33 .* limit of 32"):
        m.score_continuations(ctx, torch.randint(7, 11, (2, 3, 14)))              # l_max = 32
    m.score_continuations(ctx, torch.randint(7, 11, (2, 3, 13)))                  # 20 + 13 - 1 = 32 fits
    with pytest.raises(ValueError, match="vocab_size"):
        m.score_continuations(ctx, cont, vocab_size=17)
    with pytest.raises(ValueError, match="token ids"):
        m.score_continuations(ctx, cont, vocab_size=10)                           # tokens up to 10
    with pytest.raises(ValueError, match="token ids"):
        m.score_continuations(ctx, cont.clone().fill_(16))
