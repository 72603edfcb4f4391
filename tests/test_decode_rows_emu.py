"""Cached generation for prompts of different lengths (csrc/decode_kernels.h *_rows kernels, HyenaDecodeState's ragged mode,
generate(lengths=...)) under tests/hipemu: the per-row kernels against an fp64 direct sum, uniform positions against the single-position
kernels bit for bit, parked rows, the operator and the LM against every row run alone through the single-position path, the refusals."""
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SOURCES = [os.path.join(ROOT, "hyena_dna_amd", "csrc", "decode_kernels.h"), os.path.join(ROOT, "include", "hyena_decode.h"),
               os.path.join(ROOT, "hyena_dna_amd", "csrc", "cm.hip")]


@pytest.fixture()
def decode_emu(emu_backend):
    """the emulation library of emu_backend, rebuilt if the decode kernels are newer than it (build_emu's freshness check does not list them)"""
    from tests.hipemu import build_emu
    if not os.path.exists(build_emu.OUT) or any(os.path.getmtime(f) > os.path.getmtime(build_emu.OUT) for f in NEW_SOURCES):
        build_emu.build(force=True)
        emu_backend._lib = None
    return emu_backend


def _layer(l_max, **kw):
    d = dict(l_max=l_max, order=2, filter_order=64, emb_dim=5, short_filter_order=3, modulate=True, w=10, lr=6e-4, wd=0.0, lr_pos_emb=0.0)
    d.update(kw)
    return d


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _sc64(xm2, xm1, xn, t, w, b, bin_):
    x0 = (xm2 + bin_) if t >= 2 else torch.zeros_like(xn)
    x1 = (xm1 + bin_) if t >= 1 else torch.zeros_like(xn)
    return b + w[:, 0:1] * x0 + w[:, 1:2] * x1 + w[:, 2:3] * (xn + bin_)


def _inputs(_lib, D, B, Lcap, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    lda = _lib.row_pitch(Lcap)
    k = torch.zeros(D, lda)[:, :Lcap]                                      # (rows pitched to 64 words, as the decode cache keeps them)
    k.copy_(torch.randn(D, Lcap, generator=g) * torch.exp(-3.0 * torch.linspace(0, 1, Lcap))[None])
    return dict(k=k, lda=lda, fb=torch.randn(D, generator=g), w=torch.randn(3 * D, 3, generator=g) * 0.5, b=torch.randn(3 * D, generator=g) * 0.2,
                bin=torch.randn(3 * D, generator=g) * 0.3, hist=torch.randn(B, D, lda, generator=g).to(dtype),
                tail=torch.randn(3 * D, B, 2, generator=g).to(dtype).float(), x2=torch.randn(B, 3 * D, generator=g).to(dtype))


def _run_rows(_lib, a, pos, B, D, Lcap, dtype):
    """one step through the three *_rows entry points on copies of the state; z and the partials start from NaN (nothing unwritten may be read)"""
    hist, tail, pos = a["hist"].clone(), a["tail"].clone(), pos.clone()
    x0 = torch.full((B, D), float("nan"))
    z = torch.full((B, D), float("nan"), dtype=dtype)
    part = _lib.decode_partials(B, D, Lcap, "cpu").fill_(float("nan"))
    _lib.decode_pre_rows(a["x2"], a["bin"], a["w"], a["b"], tail, hist, x0, pos, Lcap)
    _lib.decode_conv_rows(a["k"], hist, part, pos, B, Lcap)
    _lib.decode_post_rows(part, hist, a["fb"], x0, z, pos, B, Lcap)
    return hist, tail, pos, x0, z, part


# ---- 1. the kernels against the fp64 direct sum, per row ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D,B,Lcap,ts", [(4, 3, 577, (0, 5, 576)), (4, 3, 577, (300, 300, 2)), (2, 2, 8200, (8191, 8192))])
def test_rows_kernels_vs_direct_sum(decode_emu, dtype, D, B, Lcap, ts):
    _lib = decode_emu
    a = _inputs(_lib, D, B, Lcap, dtype, D * 1000 + Lcap + ts[0])
    hist, tail, pos, x0, z, part = _run_rows(_lib, a, torch.tensor(ts, dtype=torch.int32), B, D, Lcap, dtype)
    assert pos.tolist() == [t + 1 for t in ts]                              # every valid row advanced by one
    tol = 1e-5 if dtype == torch.float32 else (2 ** -7 if dtype == torch.bfloat16 else 2 ** -10)
    w, b, bin_, k, fb, x2 = a["w"], a["b"], a["bin"], a["k"], a["fb"], a["x2"]
    for r, t in enumerate(ts):
        c = [_sc64(a["tail"][sl, r:r + 1, 0].double(), a["tail"][sl, r:r + 1, 1].double(), x2[r:r + 1, sl].double().T, t, w[sl].double(),
                   b[sl].double()[:, None], bin_[sl].double()[:, None])[:, 0] for sl in (slice(0, D), slice(D, 2 * D), slice(2 * D, 3 * D))]   # (D,) each
        assert _rel(hist[r, :, t], c[1] * c[2]) < tol
        # the tail shifted per row; only column t_b of row b's history changed
        assert torch.equal(tail[:, r, 0], a["tail"][:, r, 1]) and torch.equal(tail[:, r, 1], x2[r].float())
        other = torch.ones(a["lda"], dtype=torch.bool)
        other[t] = False
        assert torch.equal(hist[r][:, other], a["hist"][r][:, other])
        # the causal sum over the history as the kernels see it (column t = the rounded vg_t just written)
        h = hist[r, :, :t + 1].double()
        y = (h * k[:, :t + 1].double().flip(-1)).sum(-1) + fb.double() * h[:, t]
        zr = y.to(dtype).double() * c[0]
        assert _rel(x0[r], c[0]) < 1e-5
        if dtype == torch.float32:
            assert _rel(z[r], zr) < 1e-5, (r, t, _rel(z[r], zr))
        else:                                                                                                          # one rounding of the output
            err = (z[r].double() - zr).abs()
            assert (err <= tol * zr.abs() + 1e-6 + 2 * tol * y.abs() * c[0].abs()).all(), (r, t, err.max().item())
        # one partial per chunk that starts at or below t_b; the other slots were not written
        nch = part.numel() // (B * D)
        written = ~torch.isnan(part.view(nch, B, D)[:, r])
        assert written[:t // 8192 + 1].all() and not written[t // 8192 + 1:].any()


# ---- 2. uniform positions are the single-position kernels, bit for bit --------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("t", [0, 127, 129])
def test_rows_uniform_positions_equal_single_position_kernels(decode_emu, dtype, t):
    _lib = decode_emu
    D, B, Lcap = 8, 3, 130
    a = _inputs(_lib, D, B, Lcap, dtype, 77 + t)
    hist, tail, pos, x0, z, part = _run_rows(_lib, a, torch.full((B,), t, dtype=torch.int32), B, D, Lcap, dtype)
    hist1, tail1, pos1 = a["hist"].clone(), a["tail"].clone(), torch.tensor([t], dtype=torch.int32)
    x01, z1, part1 = torch.empty(B, D), torch.empty(B, D, dtype=dtype), _lib.decode_partials(B, D, Lcap, "cpu")
    _lib.decode_pre(a["x2"], a["bin"], a["w"], a["b"], tail1, hist1, x01, pos1, Lcap)
    _lib.decode_conv(a["k"], hist1, part1, pos1, B, Lcap)
    _lib.decode_post(part1, hist1, a["fb"], x01, z1, pos1, B, Lcap)
    assert pos1.item() == t + 1 and pos.tolist() == [t + 1] * B
    assert torch.equal(z, z1) and torch.equal(hist, hist1) and torch.equal(tail, tail1) and torch.equal(x0, x01)
    assert torch.equal(part, part1)                                          # (Lcap = 130: one chunk, every slot written by both)


# ---- 3. a parked row ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rows_parked_rows_stay(decode_emu, dtype):
    _lib = decode_emu
    D, B, Lcap = 4, 3, 577
    a = _inputs(_lib, D, B, Lcap, dtype, 5)
    ts = (5, -1, Lcap)
    hist, tail, pos, x0, z, part = _run_rows(_lib, a, torch.tensor(ts, dtype=torch.int32), B, D, Lcap, dtype)
    assert pos.tolist() == [6, -1, Lcap]
    for r in (1, 2):
        assert torch.isnan(z[r].float()).all() and torch.isnan(x0[r]).all()   # untouched (they started as NaN)
        assert torch.equal(hist[r], a["hist"][r]) and torch.equal(tail[:, r], a["tail"][:, r])
        assert torch.isnan(part.view(-1, B, D)[:, r]).all()
    # row 0 is the row alone at position 5 through the single-position kernels
    one = {n: (v[:1].clone() if n in ("hist", "x2") else v) for n, v in a.items()}
    tail1, pos1 = a["tail"][:, :1].clone(), torch.tensor([5], dtype=torch.int32)
    x01, z1, part1 = torch.empty(1, D), torch.empty(1, D, dtype=dtype), _lib.decode_partials(1, D, Lcap, "cpu")
    _lib.decode_pre(one["x2"], a["bin"], a["w"], a["b"], tail1, one["hist"], x01, pos1, Lcap)
    _lib.decode_conv(a["k"], one["hist"], part1, pos1, 1, Lcap)
    _lib.decode_post(part1, one["hist"], a["fb"], x01, z1, pos1, 1, Lcap)
    assert torch.equal(z[0], z1[0]) and torch.equal(hist[0], one["hist"][0]) and torch.equal(tail[:, 0], tail1[:, 0])


# ---- 4. HyenaOperator: a right-padded prefill + steps == every row alone through the single-position path --------------------------------
def test_operator_ragged_rows_match_rows_run_alone(decode_emu):
    """Two comparisons, both against the single-position path at B = 1.  (a) The three kernels: a B = 1 cache holding row b's state (history,
    tail, position copied from the ragged cache before the step) steps through decode_pre / decode_conv / decode_post on the same x2 row;
    z must be torch.equal.  (b) End to end: row b's own unpadded prompt prefilled and stepped alone; outputs within 1e-5 (the tolerance of
    test_operator_prefill_and_steps_match_forward: the projections of a (1, len, D) and a (3, 9, D) batch are different GEMM calls)."""
    from hyena_dna_amd.hyena import HyenaOperator
    from hyena_dna_amd.inference import InferenceParams
    from hyena_dna_amd.projection import hyena_linear
    D, B, P, N = 16, 3, 9, 5
    lens = (9, 2, 1)
    torch.manual_seed(D + P)
    op = HyenaOperator(d_model=D, **_layer(P + N + 3))
    seqs = [torch.randn(1, n + N, D) for n in lens]                          # row b: its prompt and the N inputs of its steps
    u = torch.zeros(B, P, D)
    for r, n in enumerate(lens):
        u[r, :n] = seqs[r][0, :n]
        u[r, n:] = torch.randn(P - n, D)                                     # pad positions: anything -- they must not matter
    lengths = torch.tensor(lens, dtype=torch.int32)
    with torch.no_grad():
        # every row alone: the existing path, B = 1, unpadded
        alone, alone_state = [], []
        for r, n in enumerate(lens):
            ip1 = InferenceParams(max_seqlen=P + N, max_batch_size=1)
            st1 = ip1.key_value_memory_dict[op._decode_key()] = op.allocate_inference_cache(1, P + N)
            outs = [op(seqs[r][:, :n], inference_params=ip1)]
            assert not st1.ragged
            alone_state.append((st1.hist.clone(), st1.tail.clone()))
            for i in range(N):
                ip1.seqlen_offset = n + i
                outs.append(op(seqs[r][:, n + i:n + i + 1], inference_params=ip1))
            alone.append(torch.cat(outs, dim=1))
        # the padded batch
        ip = InferenceParams(max_seqlen=P + N, max_batch_size=B, lengths_per_sample=lengths)
        st = ip.key_value_memory_dict[op._decode_key()] = op.allocate_inference_cache(B, P + N)
        pre = op(u, inference_params=ip)
        assert st.ragged and st.pos_rows.tolist() == list(lens)
        for r, n in enumerate(lens):
            assert _rel(pre[r, :n], alone[r][0, :n]) < 1e-5
            assert not st.hist[r, :, n:].any()                               # the pad positions' activations are gone
            assert _rel(st.hist[r, :, :n], alone_state[r][0][0, :, :n]) < 1e-6 and _rel(st.tail[:, r], alone_state[r][1][:, 0]) < 1e-6
            if n == 1:
                assert not st.tail[:, r, 0].any()                            # the column before position 0
        for i in range(N):
            ip.seqlen_offset = P + i
            x_in = torch.cat([seqs[r][:, n + i:n + i + 1] for r, n in enumerate(lens)], dim=0)
            # (a) the kernels, row by row, against the single-position kernels on the same state and x2
            x2 = hyena_linear(x_in, op.in_proj.weight, None).reshape(B, 3 * D).contiguous()
            z1 = []
            for r in range(B):
                s1 = op.allocate_inference_cache(1, P + N)
                s1.hist.copy_(st.hist[r:r + 1])
                s1.tail.copy_(st.tail[:, r:r + 1])
                s1.pos.copy_(st.pos_rows[r:r + 1])
                z1.append(s1.step(x2[r:r + 1]).clone())
            y = op(x_in, inference_params=ip)
            assert torch.equal(st.z, torch.cat(z1, dim=0)), i
            assert st.pos_rows.tolist() == [n + i + 1 for n in lens]
            # (b) end to end
            for r, n in enumerate(lens):
                assert _rel(y[r], alone[r][0, n + i:n + i + 1]) < 1e-5, (i, r)


# ---- 5. HyenaDNALM, greedy ----------------------------------------------------------------------------------------------------------------
def _lm(L, d=64, n_layer=2, seed=0, **kw):
    from hyena_dna_amd.lm import HyenaDNALM
    torch.manual_seed(seed)
    m = HyenaDNALM(d_model=d, n_layer=n_layer, d_inner=4 * d, vocab_size=12, layer=_layer(L + 2), resid_dropout=0.0, embed_dropout=0.1,
                   pad_vocab_size_multiple=8, fused_dropout_add_ln=True, residual_in_fp32=True, **kw)
    return m.eval()


def test_lm_ragged_greedy_generate_matches_rows_generated_alone(decode_emu):
    B, P, N, pad = 3, 12, 6, 4
    lens = (12, 7, 1)
    m = _lm(P + N)
    ids = torch.randint(7, 11, (B, P), generator=torch.Generator().manual_seed(2))
    lengths = torch.tensor(lens, dtype=torch.int32)
    out = m.generate(ids, max_length=P + N, use_cache=True, lengths=lengths, pad_token_id=pad, return_dict_in_generate=True, output_scores=True)
    assert out.sequences.shape == (B, P + N) and len(out.scores) == N and out.scores[0].shape == (B, 16)
    assert torch.equal(out.lengths, lengths + N) and out.lengths.dtype == torch.int32
    for r, n in enumerate(lens):
        ref = m.generate(ids[r:r + 1, :n], max_length=n + N, return_dict_in_generate=True, output_scores=True)      # the recompute loop, alone
        for i in range(N):
            assert (_rel(out.scores[i][r], ref.scores[i][0]) < 1e-5
                    or not torch.equal(ref.sequences[0, :n + i], out.sequences[r, :n + i])), (r, i)
        assert torch.equal(out.sequences[r, :n + N], ref.sequences[0])
        assert (out.sequences[r, n + N:] == pad).all()
    plain = m.generate(ids, max_length=P + N, use_cache=True, lengths=lengths)             # the sequences alone; the default pad id is 0
    for r, n in enumerate(lens):
        assert torch.equal(plain[r, :n + N], out.sequences[r, :n + N]) and (plain[r, n + N:] == 0).all()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------
def test_ragged_refusals(decode_emu):
    m = _lm(40)
    ids = torch.randint(7, 11, (2, 6), generator=torch.Generator().manual_seed(3))
    ok = torch.tensor([6, 3], dtype=torch.int32)
    with pytest.raises(ValueError, match="use_cache=True"):
        m.generate(ids, max_length=10, lengths=ok)
    for bad in ([0, 3], [7, 3]):
        with pytest.raises(ValueError, match=r"\[1, 6\]"):
            m.generate(ids, max_length=10, use_cache=True, lengths=torch.tensor(bad, dtype=torch.int32))
    with pytest.raises(ValueError, match="int32"):
        m.generate(ids, max_length=10, use_cache=True, lengths=ok.long())
    with pytest.raises(ValueError, match="int32"):
        m.generate(ids, max_length=10, use_cache=True, lengths=ok[:1])
    with pytest.raises(ValueError, match="int32"):
        m.generate(ids, max_length=10, use_cache=True, lengths=[6, 3])
    L = decode_emu.lib()
    assert L.hyena_decode_conv_rows(None, 64, None, None, None, 1, 4, 64, 64, 0, None) == 1
    assert L.hyena_decode_pre_rows(None, 12, None, None, None, None, None, None, None, 1, 1, 4, 64, 64, 0, None) == 1
    assert L.hyena_decode_post_rows(None, None, None, None, None, None, 1, 4, 64, 64, 0, None) == 1
    # good pointers, bad sizes: the history's pitch below Lcap, an unknown dtype, B above Bcap
    buf = torch.zeros(4096)
    p = buf.data_ptr()
    assert L.hyena_decode_conv_rows(p, 64, p, p, p, 1, 4, 64, 56, 0, None) == 1
    assert L.hyena_decode_post_rows(p, p, None, p, p, p, 1, 4, 64, 64, 7, None) == 1
    assert L.hyena_decode_pre_rows(p, 12, None, p, p, p, p, p, p, 2, 1, 4, 64, 64, 0, None) == 1


# ---- 7. C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_rows_entry_points_are_declared():
    import re
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hyena_decode.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(hyena_\w+)\s*\(", text))
    assert {"hyena_decode_pre_rows", "hyena_decode_conv_rows", "hyena_decode_post_rows"} <= names
