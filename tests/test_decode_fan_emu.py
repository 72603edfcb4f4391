"""Fan-out decoding -- n continuations of one cached prompt (csrc/decode_kernels.h decode_*_fan, HyenaDecodeState(fan=n),
generate(num_return_sequences=n)) -- under tests/hipemu: the three kernels bit for bit against the single-position kernels on the replicated
history and against the fp64 direct sum, HyenaDNALM teacher forcing against every row's own full forward, seeded device sampling, the cache's
size and every refusal."""
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SOURCES = [os.path.join(ROOT, "hyena_dna_amd", "csrc", "decode_kernels.h"), os.path.join(ROOT, "hyena_dna_amd", "csrc", "cm.hip"),
               os.path.join(ROOT, "include", "hyena_decode.h")]
CHUNK = 8192
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


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


class FanCase:
    """one history of P positions per group, as the replicated batch the single-position kernels take (``full``) and as the fan layout
    (``shared`` + ``rows``)"""

    def __init__(self, _lib, D, G, n, Lcap, P, dtype, dev="cpu", seed=0):
        g = torch.Generator(device=dev).manual_seed(seed)
        B, S = G * n, P // CHUNK * CHUNK
        self.D, self.G, self.n, self.B, self.Lcap, self.P, self.S, self.dtype, self.dev, self.g = D, G, n, B, Lcap, P, S, dtype, dev, g
        ldk = _lib.row_pitch(Lcap)
        self.k = (torch.randn(D, ldk, generator=g, device=dev) * torch.exp(-3.0 * torch.linspace(0, 1, ldk, device=dev))[None])[:, :Lcap]
        self.fb = torch.randn(D, generator=g, device=dev)
        self.w = torch.randn(3 * D, 3, generator=g, device=dev) * 0.5
        self.b = torch.randn(3 * D, generator=g, device=dev) * 0.2
        self.bin = torch.randn(3 * D, generator=g, device=dev) * 0.3
        hist = torch.randn(G, D, P, generator=g, device=dev).to(dtype).repeat_interleave(n, 0)                   # (B, D, P)
        tail = torch.randn(3 * D, G, 2, generator=g, device=dev).to(dtype).float().repeat_interleave(n, 1)        # (3D, B, 2)
        self.full = torch.zeros(B, D, _lib.row_pitch(Lcap), dtype=dtype, device=dev)
        self.full[:, :, :P] = hist
        self.shared = None
        if S > 0:
            self.shared = torch.zeros(G, D, _lib.row_pitch(S), dtype=dtype, device=dev)
            self.shared[:, :, :S] = hist[::n, :, :S]
        self.rows = torch.zeros(B, D, _lib.row_pitch(Lcap - S), dtype=dtype, device=dev)
        self.rows[:, :, :P - S] = hist[:, :, S:]
        self.tail_one, self.tail_fan = tail.clone(), tail.clone()
        self.pos_one = torch.tensor([P], dtype=torch.int32, device=dev)
        self.pos_fan = self.pos_one.clone()
        self.part_one, self.part_fan = _lib.decode_partials(B, D, Lcap, dev), _lib.decode_partials(B, D, Lcap, dev)

    def new_x2(self):
        return torch.randn(self.B, 3 * self.D, generator=self.g, device=self.dev).to(self.dtype)

    def step_one(self, _lib, x2):
        x0, z = torch.empty(self.B, self.D, device=self.dev), torch.empty(self.B, self.D, dtype=self.dtype, device=self.dev)
        self.part_one.fill_(float("nan"))                       # a slot that was not written in this step must never be read
        _lib.decode_pre(x2, self.bin, self.w, self.b, self.tail_one, self.full, x0, self.pos_one, self.Lcap)
        _lib.decode_conv(self.k, self.full, self.part_one, self.pos_one, self.B, self.Lcap)
        _lib.decode_post(self.part_one, self.full, self.fb, x0, z, self.pos_one, self.B, self.Lcap)
        return z, x0

    def step_fan(self, _lib, x2):
        x0, z = torch.empty(self.B, self.D, device=self.dev), torch.empty(self.B, self.D, dtype=self.dtype, device=self.dev)
        self.part_fan.fill_(float("nan"))
        _lib.decode_pre_fan(x2, self.bin, self.w, self.b, self.tail_fan, self.rows, x0, self.pos_fan, self.Lcap, self.S)
        _lib.decode_conv_fan(self.k, self.shared, self.rows, self.part_fan, self.pos_fan, self.B, self.n, self.Lcap, self.S)
        _lib.decode_post_fan(self.part_fan, self.rows, self.fb, x0, z, self.pos_fan, self.B, self.n, self.Lcap, self.S)
        return z, x0

    def assert_steps_bitwise(self, _lib, steps):
        for i in range(steps):
            t = self.P + i
            x2 = self.new_x2()
            z1, g1 = self.step_one(_lib, x2)
            z2, g2 = self.step_fan(_lib, x2)
            assert torch.equal(z1, z2) and not torch.isnan(z2.float()).any(), t
            assert torch.equal(g1, g2), t
            assert torch.equal(self.tail_one, self.tail_fan), t
            assert torch.equal(self.full[:, :, t], self.rows[:, :, t - self.S]), t
            assert torch.equal(self.pos_one, self.pos_fan) and self.pos_fan.item() == t + 1
        # nothing but the new columns was written, and the shared history not at all
        assert torch.equal(self.full[:, :, self.S:self.Lcap], self.rows[:, :, :self.Lcap - self.S])
        if self.shared is not None:
            assert torch.equal(self.full[::self.n, :, :self.S], self.shared[:, :, :self.S])


def direct_sum_check(c, z, x0, x2, tail_in, row, t):
    """tests/test_decode_emu.py test_decode_kernels_vs_direct_sum's fp64 reference and tolerances, for row ``row`` of a fan step at position t
    (the history as the kernels see it: the shared columns, then the row's own, column t being the vg_t just written)"""
    D, dtype, S = c.D, c.dtype, c.S
    cc = []
    for sl in (slice(0, D), slice(D, 2 * D), slice(2 * D, 3 * D)):
        xm2, xm1, xn = tail_in[sl, row, 0].double(), tail_in[sl, row, 1].double(), x2[row, sl].double()
        bi, ww = c.bin[sl].double(), c.w[sl].double()
        x0v = xm2 + bi if t >= 2 else torch.zeros_like(xn)
        x1v = xm1 + bi if t >= 1 else torch.zeros_like(xn)
        cc.append(c.b[sl].double() + ww[:, 0] * x0v + ww[:, 1] * x1v + ww[:, 2] * (xn + bi))
    tol = 1e-5 if dtype == torch.float32 else (2 ** -7 if dtype == torch.bfloat16 else 2 ** -10)
    assert _rel(c.rows[row, :, t - S], cc[1] * cc[2]) < tol
    assert _rel(x0[row], cc[0]) < 1e-5
    y = torch.zeros(D, dtype=torch.float64, device=c.dev)
    for s0 in range(0, t + 1, 1 << 16):                       # fp64 direct sum in slices (memory)
        s1 = min(t + 1, s0 + (1 << 16))
        parts = []
        if s0 < S:
            parts.append(c.shared[row // c.n, :, s0:min(s1, S)])
        if s1 > S:
            parts.append(c.rows[row, :, max(s0, S) - S:s1 - S])
        h = torch.cat(parts, dim=-1).double()
        y += (h * c.k[:, t - s1 + 1:t - s0 + 1].double().flip(-1)).sum(-1)
    y += c.fb.double() * c.rows[row, :, t - S].double()
    zr = y.to(dtype).double() * cc[0]
    if dtype == torch.float32:
        assert _rel(z[row], zr) < 1e-5, (row, t, _rel(z[row], zr))
    else:
        err = (z[row].double() - zr).abs()
        assert (err <= tol * zr.abs() + 1e-6 + 2 * tol * y.abs() * cc[0].abs()).all(), (row, t, err.max().item())


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Lcap,P", [(8300, 100), (8300, 8192), (8300, 8200), (16500, 16389)])
def test_fan_kernels_equal_single_position_kernels_on_replicated_history(decode_emu, dtype, Lcap, P):
    c = FanCase(decode_emu, D=3, G=2, n=3, Lcap=Lcap, P=P, dtype=dtype, seed=Lcap + P)
    assert c.S == {100: 0, 8192: 8192, 8200: 8192, 16389: 16384}[P]
    c.assert_steps_bitwise(decode_emu, 5)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fan_kernels_vs_direct_sum(decode_emu, dtype):
    c = FanCase(decode_emu, D=3, G=2, n=3, Lcap=16500, P=16389, dtype=dtype, seed=7)
    for t in (c.P, c.P + 1):
        x2, tail_in = c.new_x2(), c.tail_fan.clone()
        z, x0 = c.step_fan(decode_emu, x2)
        assert c.pos_fan.item() == t + 1
        assert torch.equal(c.tail_fan[:, :, 0], tail_in[:, :, 1]) and torch.equal(c.tail_fan[:, :, 1], x2.float().T)
        for row in range(c.B):
            direct_sum_check(c, z, x0, x2, tail_in, row, t)


def test_fan_c_abi_refuses_bad_arguments(decode_emu):
    _lib = decode_emu
    L = _lib.lib()
    D, B, fan, Lcap, S = 2, 4, 2, 8300, 8192
    k = torch.zeros(D, _lib.row_pitch(Lcap))
    hs, hr = torch.zeros(B // fan, D, _lib.row_pitch(S)), torch.zeros(B, D, _lib.row_pitch(Lcap - S))
    part, pos = _lib.decode_partials(B, D, Lcap, "cpu"), torch.tensor([-1], dtype=torch.int32)         # (a parked position: a good call does nothing)
    x, w, b, tail, x0, z = torch.zeros(B, 3 * D), torch.zeros(3 * D, 3), torch.zeros(3 * D), torch.zeros(3 * D, B, 2), torch.zeros(B, D), torch.zeros(B, D)
    p = lambda t: t.data_ptr()

    def conv(B=B, fan=fan, Lcap=Lcap, S=S, lds=hs.stride(1), ldr=hr.stride(1), hs_ptr=p(hs), hr_ptr=p(hr)):
        return L.hyena_decode_conv_fan(p(k), k.stride(0), hs_ptr, hr_ptr, p(part), p(pos), B, fan, D, Lcap, S, lds, ldr, 0, None)

    def pre(B=B, Lcap=Lcap, S=S, ldr=hr.stride(1)):
        return L.hyena_decode_pre_fan(p(x), 3 * D, None, p(w), p(b), p(tail), p(hr), p(x0), p(pos), B, B, D, Lcap, S, ldr, 0, None)

    def post(B=B, fan=fan, Lcap=Lcap, S=S, ldr=hr.stride(1)):
        return L.hyena_decode_post_fan(p(part), p(hr), None, p(x0), p(z), p(pos), B, fan, D, Lcap, S, ldr, 0, None)

    assert conv() == 0 and pre() == 0 and post() == 0 and pos.item() == -1
    assert conv(S=100) == 1 and pre(S=100) == 1 and post(S=100) == 1                        # S not a multiple of 8192
    assert conv(B=5) == 1 and post(B=5) == 1 and conv(B=3) == 1                             # B not a multiple of the fan
    assert conv(S=16384) == 1 and pre(S=16384) == 1 and post(S=16384) == 1                  # S > Lcap
    assert conv(fan=0) == 1 and post(fan=0) == 1
    assert conv(lds=S + 4) == 1 and conv(ldr=hr.stride(1) + 4) == 1 and pre(ldr=hr.stride(1) + 4) == 1 and post(ldr=12) == 1    # pitches
    assert conv(hs_ptr=p(hs) + 4) == 1 and conv(hr_ptr=p(hr) + 4) == 1 and conv(hs_ptr=None) == 1                               # pointers
    hr0 = torch.zeros(B, D, _lib.row_pitch(Lcap))
    assert conv(S=0, hs_ptr=None, lds=0, hr_ptr=p(hr0), ldr=hr0.stride(1)) == 0             # S = 0 needs no shared history ...
    assert conv(S=0, hs_ptr=None, lds=0) == 1                                               # ... but a row history of Lcap - S columns
    assert conv(Lcap=(1 << 20) + 1) == 1


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


def test_fan_cache_size(decode_emu):
    from hyena_dna_amd.hyena import HyenaOperator
    _lib = decode_emu
    torch.manual_seed(0)
    D, G, fan, P, L = 8, 2, 8, 16384, 16448
    op = HyenaOperator(d_model=D, **_layer(L))
    st = op.allocate_inference_cache(G * fan, L, dtype=torch.bfloat16, fan=fan, prompt_len=P)
    assert st.S == 16384 and st.hist_shared.shape[0] == G and st.hist.shape[0] == G * fan
    assert st.hist_shared.numel() + st.hist.numel() == G * D * _lib.row_pitch(P) + G * fan * D * _lib.row_pitch(L - P)
    hist = [v for v in vars(st).values() if torch.is_tensor(v) and v.dtype == st.dtype and v.numel() >= D * (L - P)]
    assert sum(v.numel() for v in hist) == st.hist_shared.numel() + st.hist.numel()          # and no other tensor of that size
    one = op.allocate_inference_cache(2, 64)                                                 # fan = 1: today's layout
    assert one.fan == 1 and one.S == 0 and one.hist_shared is None and one.hist.shape == (2, D, _lib.row_pitch(64))


def test_lm_fan_cached_logits_match_each_rows_full_forward(decode_emu):
    """teacher forcing: G = 2 prompts of 8200 tokens, n = 2 rows each with their own 4 next tokens; every row's logits at positions
    P - 1 ... P + 3 against one plain forward over that row's own P + 4 tokens"""
    from hyena_dna_amd.inference import InferenceParams
    G, n, P, N = 2, 2, 8200, 4
    B = G * n
    m = _lm(P + N, d=64, n_layer=1)
    gen = torch.Generator().manual_seed(3)
    prompts = torch.randint(7, 11, (G, P), generator=gen)
    cont = torch.stack([torch.randperm(4, generator=gen) + 7 for _ in range(N)], dim=1)        # (4 rows, N): distinct tokens per row at every step
    with torch.no_grad():
        ip = InferenceParams(max_seqlen=P + N, max_batch_size=B)
        ip.key_value_memory_dict = m.allocate_inference_cache(B, P + N, fan=n, prompt_len=P)
        st = next(iter(ip.key_value_memory_dict.values()))
        assert st.S == 8192 and st.hist_shared.shape[0] == G
        outs = [m(prompts, inference_params=ip)[0].logits[:, -1:].repeat_interleave(n, 0)]
        for i in range(N):
            ip.seqlen_offset = P + i
            outs.append(m(cont[:, i:i + 1], inference_params=ip)[0].logits)
        got = torch.cat(outs, dim=1)                                                          # (B, N + 1, V)
        for r in range(B):
            ref = m(torch.cat([prompts[r // n], cont[r]])[None])[0].logits[0, P - 1:P + N]
            for i in range(N + 1):
                assert _rel(got[r, i], ref[i]) < 1e-5, (r, i, _rel(got[r, i], ref[i]))


SEED = 5


def test_generate_num_return_sequences_device_sampler(decode_emu):
    G, n, P, N = 2, 4, 40, 16
    m = _lm(P + N)
    ids = torch.randint(7, 11, (G, P), generator=torch.Generator().manual_seed(4))
    kw = dict(max_length=P + N, use_cache=True, num_return_sequences=n, sampler="device", top_k=4, return_dict_in_generate=True,
              output_scores=True)
    a = m.generate(ids, seed=SEED, **kw)
    b = m.generate(ids, seed=SEED, **kw)
    assert a.sequences.shape == (G * n, P + N) and len(a.scores) == N and a.scores[0].shape[0] == G * n
    assert torch.equal(a.sequences, b.sequences) and torch.equal(torch.stack(a.scores), torch.stack(b.scores))
    assert torch.equal(a.sequences[:, :P], ids.repeat_interleave(n, 0))
    scores = torch.stack(a.scores, dim=1)                                                    # (B, N, V)
    with torch.no_grad():
        for r in range(G * n):
            ref = m(a.sequences[r:r + 1])[0].logits[0, P - 1:P + N - 1]
            for i in range(N):
                assert _rel(scores[r, i], ref[i]) < 1e-5, (r, i, _rel(scores[r, i], ref[i]))
    for g in range(G):                                                                       # the draw depends on the row
        grp = a.sequences[g * n:(g + 1) * n]
        assert not all(torch.equal(grp[0], grp[j]) for j in range(1, n)), g
    kw["top_k"] = 1
    greedy = m.generate(ids, seed=SEED, **kw).sequences
    one = m.generate(ids, max_length=P + N, use_cache=True, sampler="device", top_k=1)
    for g in range(G):
        for j in range(n):
            assert torch.equal(greedy[g * n + j], greedy[g * n]) and torch.equal(greedy[g * n + j], one[g])


def test_generate_num_return_sequences_torch_sampler(decode_emu):
    G, n, P, N = 2, 3, 20, 6
    m = _lm(P + N)
    ids = torch.randint(7, 11, (G, P), generator=torch.Generator().manual_seed(6))
    out = m.generate(ids, max_length=P + N, use_cache=True, num_return_sequences=n, return_dict_in_generate=True, output_scores=True)
    one = m.generate(ids, max_length=P + N, use_cache=True)
    assert out.sequences.shape == (G * n, P + N) and len(out.scores) == N and out.scores[0].shape[0] == G * n
    assert torch.equal(out.sequences, one.repeat_interleave(n, 0))                            # greedy
    assert m.generate(ids, max_length=P, use_cache=True, num_return_sequences=n).shape == (G * n, P)
    torch.manual_seed(1)
    smp = m.generate(ids, max_length=P + N, use_cache=True, num_return_sequences=n, top_k=4)
    assert smp.shape == (G * n, P + N) and torch.equal(smp[:, :P], ids.repeat_interleave(n, 0))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_fan_refusals(decode_emu):
    from hyena_dna_amd.hyena import HyenaOperator
    from hyena_dna_amd.inference import InferenceParams
    m = _lm(40)
    ids = torch.randint(7, 11, (2, 8), generator=torch.Generator().manual_seed(0))
    with pytest.raises(ValueError, match="use_cache"):
        m.generate(ids, max_length=12, num_return_sequences=2)
    for bad in (0, -1):
        with pytest.raises(ValueError, match="num_return_sequences"):
            m.generate(ids, max_length=12, use_cache=True, num_return_sequences=bad)
    lengths = torch.tensor([8, 5], dtype=torch.int32)
    for sampler in ("torch", "device"):
        with pytest.raises(NotImplementedError, match="out of scope"):
            m.generate(ids, max_length=12, use_cache=True, num_return_sequences=2, lengths=lengths, sampler=sampler)
    torch.manual_seed(0)
    op = HyenaOperator(d_model=8, **_layer(64))
    with pytest.raises(ValueError, match="multiple"):
        op.allocate_inference_cache(5, 32, fan=2, prompt_len=8)
    with pytest.raises(ValueError, match="prompt_len"):
        op.allocate_inference_cache(4, 32, fan=2)
    with pytest.raises(ValueError, match="prompt_len"):
        op.allocate_inference_cache(4, 32, fan=2, prompt_len=33)
    with pytest.raises(ValueError, match="fan"):
        op.allocate_inference_cache(4, 32, fan=0)
    ip = InferenceParams(max_seqlen=32, max_batch_size=4)
    ip.key_value_memory_dict[op._decode_key()] = op.allocate_inference_cache(4, 32, fan=2, prompt_len=8)
    u = torch.randn(4, 8, 8)
    with torch.no_grad():
        for rows in (4, 1, 3):
            with pytest.raises(ValueError, match="exactly 2 prompts"):
                op(u[:rows], inference_params=ip)
        with pytest.raises(ValueError, match="positions"):
            op(u[:2, :7], inference_params=ip)                                                # not the prompt length the cache was laid out for
        op(u[:2], inference_params=ip)
        ip.seqlen_offset = 8
        with pytest.raises(ValueError, match="all 4 rows"):
            op(u[:2, :1], inference_params=ip)
        op(u[:, :1], inference_params=ip)
    ragged = InferenceParams(max_seqlen=32, max_batch_size=4, lengths_per_sample=torch.tensor([8, 5], dtype=torch.int32))
    ragged.key_value_memory_dict[op._decode_key()] = op.allocate_inference_cache(4, 32, fan=2, prompt_len=8)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="out of scope"):
        op(u[:2], inference_params=ragged)
