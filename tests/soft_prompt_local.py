"""Element-wise fp64 references, derived bounds and the shared cases for the soft-prompt forms of the first block's norm, csrc/block_kernels.h
soft_embed_add_norm_fwd_kernel / soft_embed_add_norm_bwd_kernel, called ON THEIR OWN through the C ABI (include/hyena_block.h
hyena_soft_embed_add_norm_*) on caller-made buffers, the row-wise head (row_head_kernel, hyena_row_head_*), and the model-level checks of HyenaDNALM's soft-token route and soft_prompt.SoftPromptLM.
Shared by tests/test_soft_prompt_emu.py (CPU emulation of the kernels) and tests/test_gpu_soft_prompt.py (gfx950).  Not a test file.

Built from tests/block_local.py (notation, Philox restatement, fwd64 / bwd64 and their error recurrences, Guarded buffers, _Stats):

Forward.  Row (b, t) of the (B, n + L, D) output has x0 = keep2 ks2 soft[t] (t < n) or table[ids[b, t - n]] (t >= n), then r = keep ks x0 and
block_local's recurrences from r on.  c_r, the roundings of r, is (p > 0) for a token row and (p > 0) + (soft_p > 0) for a soft row: one per
scaling.  fwd64 counts c_r = (keep given) + (residual given), so the soft rows with a soft dropout are taken from a second evaluation with a
residual of exact zeros, which changes no value and adds the one rounding (e_r = gamma_(c_r) |r|).

Backward.  dr and dx = keep ks dr of every soft row exactly as bwd64 states them (E_dx inherited), then

    d_soft[t] = keep2[t] ks2 sum_b dx[b, t]          |got - ref64| <= gamma_(B + c) (S + H) + H,   S = sum_b |term|, H = sum_b ks2 keep2 E_dx

with term = keep2 ks2 dx[b, t] and c = (soft_p > 0): B - 1 additions (the bound allows B) and the one scaling.  The operands are block_local's
structured draws (|dr| stays near q >= 1), so with B <= 3 the bound stays far below the smallest non-zero term -- asserted as `margin` < 1 for every
case, and checked for the references alone, without any kernel, by the emulator file."""
import torch
import torch.nn.functional as F

from tests import block_local as BL
from tests.block_local import (BAD_ID, BLK_VMAX, DTYPES, EPS, NAME, NAN, SEED, Guarded, _mag, _out, _p, _same, _Stats, bwd64, draw_gw, draw_ids,
                               draw_params, draw_rows, dropout_params, f32, fwd64, gamma, half_ulp_io, keep_mask, philox_words)  # noqa: F401

SOFT_SEED = 0x0FED_CBA9_8765_4321
SOFT_D = [64, 128, 256]                                              # E = 1, 2 (a lane holds a part of a Philox group of four), 4
SOFT_V = [1, 12, 16]
SOFT_SHAPES = [(1, 1, 1), (2, 3, 7), (3, 4, 1), (2, 5, 3), (3, 37, 2)]   # (B, n, L): partial workgroups, idle wavefronts, a soft / token boundary inside a workgroup
SOFT_DROPS = [(0.0, 0.0), (0.1, 0.0), (0.0, 0.5), (0.1, 0.1)]            # (dropout_p, soft_dropout_p)
SOFT_FWD_BIG = (3, 2050, 700, 64)                                    # 8250 rows > the 2048 x 4 rows of one grid sweep
SOFT_BWD_BIG = (1, 8197, 1, 64)                                      # 8197 soft positions: a second, partial sweep of the backward's grid-stride loop


def soft_cases(D, V):
    """every shape at one (D, V); output / dout type, the two dropouts and the presence of d_residual_out cycle so that every D meets every pair of
    dropouts and every type"""
    i = SOFT_D.index(D) + SOFT_V.index(V)
    for k, (B, n, L) in enumerate(SOFT_SHAPES):
        j = i + k
        p, sp = SOFT_DROPS[(j + SOFT_V.index(V)) % 4]
        yield dict(B=B, n=n, L=L, D=D, V=V, OT=DTYPES[(j + k // 3) % 3], p=p, sp=sp, with_h=bool((j + k // 2) % 2), seed=300 * D + 10 * n + V + k)


def big_cases():
    B, n, L, D = SOFT_FWD_BIG
    yield dict(B=B, n=n, L=L, D=D, V=12, OT=torch.bfloat16, p=0.1, sp=0.1, with_h=True, seed=2050)
    B, n, L, D = SOFT_BWD_BIG
    yield dict(B=B, n=n, L=L, D=D, V=16, OT=torch.float16, p=0.1, sp=0.5, with_h=False, seed=8197)


def all_cases():
    for D in SOFT_D:
        for V in SOFT_V:
            yield from soft_cases(D, V)
    yield from big_cases()


def soft_keep(sp, n, D, dev):
    """the soft tokens' mask, per element of (n, D) from (SOFT_SEED, t D + c): (keep fp64 0 / 1 or None, keep_scale)"""
    if sp == 0.0:
        return None, 1.0
    thr, ks = dropout_params(sp)
    return (philox_words(SOFT_SEED, n * D, dev) >= thr).double().reshape(n, D), ks


def _seeds(dev, p, sp):
    sd = torch.tensor([SEED], dtype=torch.int64, device=dev) if p > 0.0 else None
    ss = torch.tensor([SOFT_SEED], dtype=torch.int64, device=dev) if sp > 0.0 else None
    return sd, ss


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---- operands and references (no kernel involved) ----------------------------------------------------------------------------------------------
def draw_forward(B, n, L, D, V, p, sp, g, dev):
    amp = 1.0 if p == 0.0 and sp == 0.0 else 2.0                     # a dropped element sits at 0: keep it away from the row mean
    soft = draw_rows((n,), D, g, amp=amp)[0].float().to(dev)
    table = draw_rows((V,), D, g, amp=amp)[0].float().to(dev)
    ids = draw_ids(B * L, V, g).view(B, L).to(dev)
    return soft, table, ids


def forward_ref(soft, table, ids, w, b, p, sp):
    """references and bounds of the four forward outputs over the (B, n + L) rows"""
    dev = soft.device
    (B, L), (n, D) = ids.shape, soft.shape
    keep2, ks2 = soft_keep(sp, n, D, dev)
    s64 = soft.double() if keep2 is None else keep2 * ks2 * soft.double()
    safe = ids.clamp(0, table.shape[0] - 1)
    x64 = torch.cat([s64.unsqueeze(0).expand(B, n, D), table.double()[safe]], 1)
    keep, ks = keep_mask(p, (B, n + L, D), dev)
    R = fwd64(x64, None, w.double(), b.double(), keep, ks)
    if keep2 is not None:                                            # the soft rows carry one rounding more (module docstring)
        R2 = fwd64(x64, torch.zeros_like(x64), w.double(), b.double(), keep, ks)
        is_soft = torch.arange(n + L, device=dev) < n
        for k in R:
            m = is_soft[None, :, None] if R[k].dim() == 3 else is_soft[None, :]
            R[k] = torch.where(m, R2[k], R[k])
    return R


def draw_backward(B, n, L, D, OT, with_h, w, g, dev):
    """caller-made saved / mean / rstd / dout / h over all B (n + L) rows: structured draws in the soft rows, NaN in the token rows (not read)"""
    sv64, tau, q, sigma = draw_rows((B, n), D, g)
    saved_s = sv64.float().to(dev)
    s64 = saved_s.double()
    mu_s = s64.mean(-1).float()
    rs_s = ((s64 - s64.mean(-1, keepdim=True)) ** 2).mean(-1).add(f32(EPS)).rsqrt().float()
    dout_s = (draw_gw(tau, q, sigma, g, (B, n)).to(dev) / w.double()).to(OT)
    h_s = (sigma * _mag((B, n, D), g, 0.5)).float().to(dev) if with_h else None

    def full(x, dtype, tail):
        t = torch.full((B, n + L) + tail, NAN, dtype=dtype, device=dev)
        t[:, :n] = x
        return t
    full_ = dict(saved=full(saved_s, torch.float32, (D,)), mean=full(mu_s, torch.float32, ()), rstd=full(rs_s, torch.float32, ()),
                 dout=full(dout_s, OT, (D,)), h=None if h_s is None else full(h_s, torch.float32, (D,)))
    return dict(saved=saved_s, mean=mu_s, rstd=rs_s, dout=dout_s, h=h_s), full_


def backward_ref(soft_rows, w, p, sp, B, n, L, D):
    """(terms (B, n, D), H (B, n, D), c) of d_soft = sum over b of terms"""
    dev = w.device
    keep, ks = keep_mask(p, (B, n + L, D), dev)
    keep_s = None if keep is None else keep[:, :n].reshape(B * n, D)
    h = soft_rows["h"]
    Rb = bwd64(soft_rows["dout"].double().reshape(B * n, D), soft_rows["saved"].double().reshape(B * n, D), soft_rows["mean"].double().reshape(-1),
               soft_rows["rstd"].double().reshape(-1), w.double(), None if h is None else h.double().reshape(B * n, D), keep_s, ks)
    keep2, ks2 = soft_keep(sp, n, D, dev)
    scale = 1.0 if keep2 is None else keep2 * ks2
    return scale * Rb["dx"].view(B, n, D), scale * Rb["E_dx"].view(B, n, D), int(keep2 is not None)


def reference_margin(B, n, L, D, V, OT, p, sp, with_h, seed, dev=torch.device("cpu")):
    """the largest ratio of d_soft's bound to the smallest non-zero term of the same sum, from the references alone"""
    g = torch.Generator().manual_seed(seed)
    w, _ = draw_params(D, g, dev)
    draw_forward(B, n, L, D, V, p, sp, g, dev)                        # (the generator's state as run_soft leaves it)
    soft_rows, _ = draw_backward(B, n, L, D, OT, with_h, w, g, dev)
    terms, H, c = backward_ref(soft_rows, w, p, sp, B, n, L, D)
    bound = BL.sum_bound(terms.abs().sum(0), H.sum(0), B, c)
    small = torch.where(terms != 0, terms.abs(), torch.full_like(terms, float("inf"))).amin(0)
    return float((bound / small).max())


# ---- the two kernels through the C ABI ---------------------------------------------------------------------------------------------------------
def _fwd_call(_lib, dev, ib, tb, sb, wb, bb, V, OT, p, sp, B, n, L, D):
    sd, ss = _seeds(dev, p, sp)
    rows = B * (n + L)
    o = (_out((rows, D), OT, dev), _out((rows, D), torch.float32, dev), _out((rows,), torch.float32, dev), _out((rows,), torch.float32, dev))
    _lib.check(_lib.lib().hyena_soft_embed_add_norm_fwd(ib.ptr, tb.ptr, V, sb.ptr, sp, _ptr(ss), wb.ptr, bb.ptr, EPS, p, _ptr(sd), o[0].ptr, _lib.dtype_code(OT),
                                                        o[1].ptr, o[2].ptr, o[3].ptr, B, n, L, D, _lib._backend.stream(dev)))
    assert all(t.guards_intact() for t in o), "a guard row of a forward output was written"
    return o


def _bwd_call(_lib, dev, bufs, wb, OT, p, sp, B, n, L, D):
    sd, ss = _seeds(dev, p, sp)
    gb, hb, vb, mb, rb = bufs
    o = _out((n, D), torch.float32, dev)
    _lib.check(_lib.lib().hyena_soft_embed_add_norm_bwd(gb.ptr, _lib.dtype_code(OT), _p(hb), vb.ptr, wb.ptr, mb.ptr, rb.ptr, p, _ptr(sd), sp, _ptr(ss), o.ptr,
                                                        B, n, L, D, _lib._backend.stream(dev)))
    return o


def _table_buf(table, dev):
    V, D = table.shape
    tb = Guarded((BLK_VMAX, D), torch.float32, dev, NAN)             # rows [V, 16) and the guards: NaN
    tb.t[:V] = table
    return tb


def run_soft(_lib, dev, B, n, L, D, V, OT, p, sp, with_h, seed=0, label="", wrappers=True):
    """both kernels on caller-made buffers: every element within its bound, NaN in what is not read, a sentinel around what is written, two runs the
    same bits, the wrappers of _lib the same bits"""
    g = torch.Generator().manual_seed(seed)
    w, b = draw_params(D, g, dev)
    soft, table, ids = draw_forward(B, n, L, D, V, p, sp, g, dev)
    sd, ss = _seeds(dev, p, sp)
    wb, bb, ib, sb, tb = Guarded.input(w), Guarded.input(b), Guarded.input(ids, BAD_ID), Guarded.input(soft), _table_buf(table, dev)
    st = _Stats()
    rows = B * (n + L)
    with _lib._backend.guard(dev):
        out, ro, mean, rstd = _fwd_call(_lib, dev, ib, tb, sb, wb, bb, V, OT, p, sp, B, n, L, D)
        assert _same((out, ro, mean, rstd), _fwd_call(_lib, dev, ib, tb, sb, wb, bb, V, OT, p, sp, B, n, L, D)), "soft_embed_add_norm_fwd is not repeatable bit for bit"
        R = forward_ref(soft, table, ids, w, b, p, sp)
        st.elem("res_out", ro, R["r"].reshape(rows, D), R["e_r"].reshape(rows, D), torch.float32)
        st.elem("mean", mean, R["mean"].reshape(rows), R["e_m"].reshape(rows), torch.float32)
        st.elem("rstd", rstd, R["rstd"].reshape(rows), R["e_s"].reshape(rows), torch.float32)
        st.elem("out", out, R["out"].reshape(rows, D), R["E_out"].reshape(rows, D), OT)
        if wrappers:
            ow = _lib.soft_embed_add_norm_fwd(ids, table, soft, w, b, EPS, OT, dropout_p=p, seed=sd, soft_dropout_p=sp, soft_seed=ss)
            assert all(torch.equal(a_, b_.t) for a_, b_ in zip(ow, (out, ro, mean, rstd))), "the wrapper's bits"
        # ---- backward
        soft_rows, full = draw_backward(B, n, L, D, OT, with_h, w, g, dev)
        bufs = (Guarded.input(full["dout"].view(rows, D)), None if full["h"] is None else Guarded.input(full["h"].view(rows, D)),
                Guarded.input(full["saved"].view(rows, D)), Guarded.input(full["mean"].view(rows)), Guarded.input(full["rstd"].view(rows)))
        ds = _bwd_call(_lib, dev, bufs, wb, OT, p, sp, B, n, L, D)
        assert _same((ds,), (_bwd_call(_lib, dev, bufs, wb, OT, p, sp, B, n, L, D),)), "soft_embed_add_norm_bwd is not repeatable bit for bit"
        terms, H, c = backward_ref(soft_rows, w, p, sp, B, n, L, D)
        st.total("d_soft", ds, terms, H, B, c)
        if wrappers:
            bw = _lib.soft_embed_add_norm_bwd(full["dout"].view(rows, D), None if full["h"] is None else full["h"].view(rows, D), full["saved"].view(rows, D), w,
                                              full["mean"].view(rows), full["rstd"].view(rows), B, n, L, dropout_p=p, seed=sd, soft_dropout_p=sp, soft_seed=ss)
            assert torch.equal(bw, ds.t), "the wrapper's bits"
    print(st.line(f"{label} soft {NAME[OT]} B={B} n={n} L={L} D={D} V={V} p={p} soft_p={sp} h={int(with_h)}"), flush=True)
    assert st["margin"] < 1.0, ("the bound of a sum exceeds its smallest term", st["margin"])
    return st


def run_cross_check_fwd(_lib, dev, B, n, L, D, V, OT, p, seed=0):
    """soft_dropout_p = 0: the four outputs equal add_norm_fwd's on the concatenated tensor with the same seed, bit for bit"""
    g = torch.Generator().manual_seed(seed)
    w, b = draw_params(D, g, dev)
    soft, table, ids = draw_forward(B, n, L, D, V, p, 0.0, g, dev)
    sd, _ = _seeds(dev, p, 0.0)
    got = _lib.soft_embed_add_norm_fwd(ids, table, soft, w, b, EPS, OT, dropout_p=p, seed=sd)
    x0 = torch.cat([soft.unsqueeze(0).expand(B, n, D), F.embedding(ids, table)], 1).reshape(B * (n + L), D).contiguous()
    want = _lib.add_norm_fwd(x0, None, w, b, EPS, OT, dropout_p=p, seed=sd)
    for name, a_, b_ in zip(("out", "res_out", "mean", "rstd"), got, want):
        assert torch.equal(a_, b_), (name, B, n, L, D, p)


def run_cross_check_bwd(_lib, dev, B, n, L, D, OT, p, with_h, seed=0):
    """soft_dropout_p = 0, B = 1 or 2: d_soft equals the soft row of add_norm_bwd's fp32 dx0, or the sum of the two rows (one addition: order-free)"""
    assert B in (1, 2)
    g = torch.Generator().manual_seed(seed)
    w, _ = draw_params(D, g, dev)
    rows = B * (n + L)
    sv64, tau, q, sigma = draw_rows((rows,), D, g)
    saved = sv64.float().to(dev)
    s64 = saved.double()
    mu = s64.mean(-1).float()
    rs = ((s64 - s64.mean(-1, keepdim=True)) ** 2).mean(-1).add(f32(EPS)).rsqrt().float()
    dout = (draw_gw(tau, q, sigma, g, (rows,)).to(dev) / w.double()).to(OT)
    h = (sigma * _mag((rows, D), g, 0.5)).float().to(dev) if with_h else None
    sd, _ = _seeds(dev, p, 0.0)
    got = _lib.soft_embed_add_norm_bwd(dout, h, saved, w, mu, rs, B, n, L, dropout_p=p, seed=sd)
    dx = _lib.add_norm_bwd(dout, h, saved, w, mu, rs, torch.float32, need_dres=False, dropout_p=p, seed=sd, offer_colsum=False)[0].view(B, n + L, D)[:, :n]
    want = dx[0] if B == 1 else dx[0] + dx[1]
    assert torch.equal(got, want), (B, n, L, D, p)


def run_bad_ids(_lib, dev, B, n, L, D, V, OT, p, sp, seed=0):
    """ids -1 and V poison their own token rows of the forward and nothing else: every other row within its bound and, bit for bit, what the same call
    gives with valid ids; d_soft from what the forward stored is finite and the same bits with and without the bad ids"""
    assert B * L >= 3
    g = torch.Generator().manual_seed(seed)
    w, b = draw_params(D, g, dev)
    soft, table, ids = draw_forward(B, n, L, D, V, p, sp, g, dev)
    bad_ids = ids.clone().view(-1)
    where = [1, B * L - 1]
    bad_ids[where[0]], bad_ids[where[1]] = -1, V
    bad_ids = bad_ids.view(B, L)
    live = torch.ones(B, n + L, dtype=torch.bool, device=dev)
    for k in where:
        live[k // L, n + k % L] = False
    live = live.view(-1)
    rows = B * (n + L)
    wb, bb, sb, tb = Guarded.input(w), Guarded.input(b), Guarded.input(soft), _table_buf(table, dev)
    res = {}
    with _lib._backend.guard(dev):
        for kind, these in (("good", ids), ("bad", bad_ids)):
            ib = Guarded.input(these, BAD_ID)
            out, ro, mean, rstd = _fwd_call(_lib, dev, ib, tb, sb, wb, bb, V, OT, p, sp, B, n, L, D)
            soft_rows, full = draw_backward(B, n, L, D, OT, True, w, torch.Generator().manual_seed(seed + 1), dev)
            # the backward on what the forward stored: residual', mean, rstd as they are (NaN in the poisoned rows)
            bufs = (Guarded.input(full["dout"].view(rows, D)), Guarded.input(full["h"].view(rows, D)), Guarded.input(ro.t.clone()), Guarded.input(mean.t.clone()),
                    Guarded.input(rstd.t.clone()))
            ds = _bwd_call(_lib, dev, bufs, wb, OT, p, sp, B, n, L, D)
            assert ds.guards_intact() and bool(torch.isfinite(ds.t).all()), "d_soft with two ids outside [0, V)"
            res[kind] = (out.t.clone(), ro.t.clone(), mean.t.clone(), rstd.t.clone(), ds.t.clone())
    out, ro, mean, rstd, ds = res["bad"]
    assert bool(torch.isnan(ro[~live]).all()) and bool(torch.isnan(out[~live].float()).all()), "a row with a bad id is not NaN"
    R = forward_ref(soft, table, ids, w, b, p, sp)
    E = R["E_out"].reshape(rows, D) + half_ulp_io(R["out"].reshape(rows, D).abs() + R["E_out"].reshape(rows, D), OT)
    assert bool(((out.double() - R["out"].reshape(rows, D)).abs() <= E)[live].all()), "a row beside a bad id"
    for name, a_, b_ in zip(("out", "res_out", "mean", "rstd"), res["bad"], res["good"]):
        assert torch.equal(a_[live], b_[live]), name + ": a row with a valid id changed"
    assert torch.equal(res["bad"][4], res["good"][4]), "d_soft changed"


def check_bad_args(_lib, dev):
    """n = 0 or a null pointer: HYENA_ERR_BAD_ARG before anything is launched.  The buffers live on `dev` and are large enough for the shapes passed
    (B = n = L = 1, D = 64, id 0 of a one-row table), so a refusal that regressed would fail its assertion here, not launch on memory of another kind."""
    L_ = _lib.lib()
    one = torch.zeros(2 * 64, dtype=torch.float32, device=dev)
    ids = torch.zeros(4, dtype=torch.int64, device=dev)
    args = lambda n, soft: (ids.data_ptr(), one.data_ptr(), 1, soft, 0.0, None, one.data_ptr(), one.data_ptr(), EPS, 0.0, None, one.data_ptr(), 0,   # noqa: E731
                            one.data_ptr(), one.data_ptr(), one.data_ptr(), 1, n, 1, 64, None)
    assert L_.hyena_soft_embed_add_norm_fwd(*args(0, one.data_ptr())) == 1
    assert L_.hyena_soft_embed_add_norm_fwd(*args(1, None)) == 1
    assert L_.hyena_soft_embed_add_norm_bwd(one.data_ptr(), 0, None, one.data_ptr(), one.data_ptr(), one.data_ptr(), one.data_ptr(), 0.0, None, 0.0, None,
                                            one.data_ptr(), 1, 0, 1, 64, None) == 1
    assert L_.hyena_soft_embed_add_norm_bwd(one.data_ptr(), 0, None, one.data_ptr(), one.data_ptr(), one.data_ptr(), one.data_ptr(), 0.0, None, 0.0, None,
                                            None, 1, 1, 1, 64, None) == 1
    assert L_.hyena_soft_embed_add_norm_fwd(*args(1, one.data_ptr())[:4], 0.5, None, *args(1, one.data_ptr())[6:]) == 1      # a dropout without its seed
    for V, D, code in ((16, 256, 1), (12, 128, 0), (17, 256, 1), (16, 512, 1), (0, 256, 1), (1, 64, 2)):
        assert L_.hyena_soft_embed_add_norm_supported(V, D, code) == L_.hyena_embed_add_norm_supported(V, D, code)


# ---- model level ---------------------------------------------------------------------------------------------------------------------------------
L_MAX = 130
MODEL_CASES = [(1, 1, 59), (2, 5, 59), (2, 1, 122), (1, 5, 122), (2, 5, 122)]       # (B, n, L): n in {1, 5}, L in {59, 122}, B in {1, 2}; totals 60 .. 127


def make_model(dev, seed=0, embed_dropout=0.1):
    import hyena_dna_amd.lm as LM
    torch.manual_seed(seed)
    layer = dict(l_max=L_MAX, order=2, filter_order=64, emb_dim=5, short_filter_order=3, modulate=True, w=10, lr=6e-4, wd=0.0, lr_pos_emb=0.0)
    m = LM.HyenaDNALM(d_model=64, n_layer=2, d_inner=128, vocab_size=12, layer=layer, resid_dropout=0.0, embed_dropout=embed_dropout,
                      pad_vocab_size_multiple=8, fused_dropout_add_ln=True, residual_in_fp32=True)
    assert m.lm_head.weight.shape == (16, 64)
    return m.to(dev)


def make_pair(dev, n, seed=0, pdrop=0.0):
    """the same frozen model behind a fused and an unfused SoftPromptLM with the same soft tokens"""
    from hyena_dna_amd.soft_prompt import SoftPromptLM
    model = make_model(dev, seed)
    torch.manual_seed(seed + 1)
    fused = SoftPromptLM(model, n, soft_token_pdrop=pdrop, fused=True)
    unfused = SoftPromptLM(model, n, soft_token_pdrop=pdrop, fused=False)
    if n > 0:
        with torch.no_grad():
            fused.soft_tokens.mul_(20.0)                             # N(0, 0.4): the soft rows matter to the logits
            unfused.soft_tokens.copy_(fused.soft_tokens)
    return model, fused.eval(), unfused.eval()


def draw_batch(dev, B, L, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(7, 11, (B, L), generator=g).to(dev)
    pos = torch.tensor(sorted({1, L // 3, L // 2, L - 1}), dtype=torch.int64, device=dev)
    return ids, pos


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _routes_seen(fn):
    """run fn() and report which of the two first-norm passes ran"""
    from hyena_dna_amd import _lib
    seen = []
    real_s = _lib.soft_embed_add_norm_fwd
    _lib.soft_embed_add_norm_fwd = lambda *a, **k: (seen.append("soft"), real_s(*a, **k))[1]
    try:
        out = fn()
    finally:
        _lib.soft_embed_add_norm_fwd = real_s
    return out, seen


def check_fused_equals_unfused_fp32(dev, B, n, L):
    """fp32, both dropouts off: logits, loss-at-positions gradient of the soft tokens bit for bit; no backbone gradient; loss() = F.cross_entropy on the
    unfused full logits at those positions"""
    model, fused, unfused = make_pair(dev, n, seed=B + n + L)
    ids, pos = draw_batch(dev, B, L, seed=L + B)
    lf, seen = _routes_seen(lambda: fused(ids))
    assert seen == ["soft"], "the fused route did not run the soft-prompt kernel"
    lu, seen = _routes_seen(lambda: unfused(ids))
    assert seen == [], "the unfused route ran the soft-prompt kernel"
    assert lf.shape == lu.shape == (B, L, 16) and torch.equal(lf, lu), "logits"
    label_pos = pos[pos >= 1]
    grads = {}
    for name, m in (("fused", fused), ("unfused", unfused)):
        m.zero_grad(set_to_none=True)
        loss = m.loss(ids, label_pos)
        want = F.cross_entropy(lu[:, label_pos - 1].float().reshape(-1, 16), ids[:, label_pos].reshape(-1))
        assert abs(loss.item() - want.item()) <= 1e-6 * abs(want.item()), (name, loss.item(), want.item())
        loss.backward()
        grads[name] = m.soft_tokens.grad.clone()
        assert bool(torch.isfinite(grads[name]).all()) and bool(grads[name].any())
        assert all(p.grad is None for p in model.parameters()), name + ": a backbone parameter received a gradient"
    assert torch.equal(grads["fused"], grads["unfused"]), "soft_tokens.grad"
    # the full-length logits' gradient too (every input position contributes)
    full = {}
    for name, m in (("fused", fused), ("unfused", unfused)):
        m.zero_grad(set_to_none=True)
        m(ids).float().square().mean().backward()
        full[name] = m.soft_tokens.grad.clone()
    assert torch.equal(full["fused"], full["unfused"]), "soft_tokens.grad of the full logits"


def _head_bound(hidden, weight):
    """two fp32 evaluations of hidden @ weight^T, each a sum of K products in some order, differ by at most 2 gamma_K sum_k |h_k w_k|"""
    K = hidden.shape[-1]
    return 2 * gamma(K) * (hidden.double().abs() @ weight.double().abs().t())


def check_hidden_at_rows(dev, B, n, L):
    """the part of hidden_at that this package computes itself: the final norm's output at `positions` is, bit for bit, the rows of the final norm's
    output over all positions (per-position kernels); the head's logits on those rows are within the fp32 bound of a K-term sum of the full logits' rows"""
    model, fused, unfused = make_pair(dev, n, seed=B + n + L)
    ids, pos = draw_batch(dev, B, L, seed=L + B)
    with torch.no_grad():
        for m in (fused, unfused):
            kw = dict(soft_tokens=m.soft_tokens, soft_fused=m.fused)
            h_all, h_at = model.hidden_at(ids, None, **kw), model.hidden_at(ids, pos, **kw)
            assert h_all.shape == (B, L, 64) and h_at.shape == (B, pos.numel(), 64) and torch.equal(h_at, h_all[:, pos])
            full, at = m(ids), m(ids, pos)
            diff = (at.double() - full[:, pos].double()).abs()
            bound = _head_bound(h_at, model.lm_head.weight)
            print(f"[soft-prompt hidden_at] B={B} n={n} L={L} fused={m.fused}: max |logits at positions - rows of the full logits| = {float(diff.max()):.3e}, "
                  f"largest share of the bound {float((diff / bound).max()):.3g}, bit-equal {torch.equal(at, full[:, pos])}", flush=True)
            assert bool((diff <= bound).all())


def check_hidden_at_plus_head_bit_for_bit(dev, B, n, L):
    """hidden_at + head against the corresponding rows of the full logits, bit for bit: the final norm is per-position (check_hidden_at_rows) and
    SoftPromptLM's head is the row-wise kernel (hyena_row_head_fwd), whose order of additions does not depend on the row count.  (Through the library
    GEMM, which picks its kernel from the row count, the same comparison was off by 1.2e-7 .. 2.4e-7, one or two units in the last place, in all
    five MODEL_CASES on gfx950.)"""
    from hyena_dna_amd import _lib
    model, fused, unfused = make_pair(dev, n, seed=B + n + L)
    ids, pos = draw_batch(dev, B, L, seed=L + B)
    calls = []
    real = _lib.row_head_fwd
    _lib.row_head_fwd = lambda *a, **k: (calls.append(a[0].shape[0]), real(*a, **k))[1]
    try:
        with torch.no_grad():
            for m in (fused, unfused):
                assert torch.equal(m(ids, pos), m(ids)[:, pos]), f"fused={m.fused}: hidden_at + head is not the rows of the full logits"
    finally:
        _lib.row_head_fwd = real
    # the row-wise head ran, on the gathered rows and on all of them (the full call keeps the soft and pad rows: its logits are sliced, not its input)
    assert calls[0::2] == [B * pos.numel()] * 2 and all(B * (n + L) <= c < B * (n + L + 64) for c in calls[1::2]) and len(calls) == 4, calls


# ---- the row-wise head ---------------------------------------------------------------------------------------------------------------------------
HEAD_ROWS = [1, 5, 37, 8197]                                        # partial workgroups; 8197: a second, partial sweep of the capped grid


def run_row_head(_lib, dev, rows, D, V, T, seed=0, label=""):
    """hyena_row_head_fwd / _bwd on caller-made buffers against fp64: a logit is E products and E - 1 + 6 additions (+ the first, onto zero), so
    |got - ref64| <= gamma_(E + 7) sum_c |x w| + half_ulp_io; dx is V products and additions: gamma_(V + 1) sum_v |dy w| + half_ulp_io.  Sentinels
    around the outputs, NaN around the inputs, two runs the same bits, and the point of the kernel: the logits of a subset of the rows, computed on
    their own, are the bits of those rows of the full call."""
    lib, code, stream = _lib.lib(), _lib.dtype_code(T), _lib._backend.stream(dev)
    g = torch.Generator().manual_seed(seed)
    E = D // 64
    x = torch.randn(rows, D, generator=g).to(T).to(dev)
    w = torch.randn(V, D, generator=g).to(T).to(dev)
    dy = torch.randn(rows, V, generator=g).to(T).to(dev)
    xb, dyb = Guarded.input(x), Guarded.input(dy)
    wb = Guarded((BLK_VMAX, D), T, dev, NAN)                         # rows [V, 16) and the guards: NaN
    wb.t[:V] = w
    st = _Stats()
    with _lib._backend.guard(dev):
        def fwd():
            o = _out((rows, V), T, dev)
            _lib.check(lib.hyena_row_head_fwd(xb.ptr, wb.ptr, o.ptr, rows, V, D, code, stream))
            return o

        def bwd():
            o = _out((rows, D), T, dev)
            _lib.check(lib.hyena_row_head_bwd(dyb.ptr, wb.ptr, o.ptr, rows, V, D, code, stream))
            return o
        out, dx = fwd(), bwd()
        assert _same((out, dx), (fwd(), bwd())), "row_head is not repeatable bit for bit"
        x64, w64, dy64 = x.double(), w.double(), dy.double()
        st.elem("logits", out, x64 @ w64.t(), gamma(E + 7) * (x64.abs() @ w64.abs().t()), T)
        st.elem("dx", dx, dy64 @ w64, gamma(V + 1) * (dy64.abs() @ w64.abs()), T)
        assert torch.equal(_lib.row_head_fwd(x, w), out.t) and torch.equal(_lib.row_head_bwd(dy, w), dx.t), "the wrapper's bits"
        pick = torch.arange(0, rows, 3, device=dev)
        assert torch.equal(_lib.row_head_fwd(x[pick].contiguous(), w), out.t[pick]), "a row's logits depend on the other rows of the call"
        assert torch.equal(_lib.row_head_bwd(dy[pick].contiguous(), w), dx.t[pick])
    print(st.line(f"{label} row_head {NAME[T]} rows={rows} D={D} V={V}"), flush=True)
    return st


def check_row_head_autograd(dev):
    """soft_prompt.row_head: F.linear's values and input gradient within the fp32 bound, no weight gradient asked for; a head that wants a gradient or
    carries a bias goes through hyena_linear"""
    from hyena_dna_amd import _lib
    from hyena_dna_amd.soft_prompt import row_head
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 7, 64, generator=g).to(dev).requires_grad_(True)
    w = torch.nn.Parameter(torch.randn(16, 64, generator=g).to(dev), requires_grad=False)
    dy = torch.randn(2, 7, 16, generator=g).to(dev)
    calls = []
    real = _lib.row_head_fwd
    _lib.row_head_fwd = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        y = row_head(x, w)
        y.backward(dy)
        assert calls == [1]
        assert bool(((y.double() - x.double() @ w.double().t()).abs() <= gamma(8) * (x.double().abs() @ w.double().abs().t())).all())
        assert bool(((x.grad.double() - dy.double() @ w.double()).abs() <= gamma(17) * (dy.double().abs() @ w.double().abs())).all())
        w.requires_grad_(True)
        bias = torch.randn(16, generator=g).to(dev)
        y2 = row_head(x, w)
        y3 = row_head(x.detach(), w.detach(), bias)
        assert calls == [1] and y2.shape == y3.shape == y.shape
        # the fallback's values: F.linear in fp64, a 64-term fp32 sum in any order (+ the bias add)
        ref2 = x.detach().double() @ w.detach().double().t()
        mag = x.detach().double().abs() @ w.detach().double().abs().t()
        assert bool(((y2.detach().double() - ref2).abs() <= gamma(64) * mag).all())
        assert bool(((y3.double() - (ref2 + bias.double())).abs() <= gamma(65) * (mag + bias.double().abs())).all())
    finally:
        _lib.row_head_fwd = real


def check_autocast(dev, B, n, L, dtype=torch.bfloat16):
    """bf16 autocast: each route against the fp32 unfused run; the fused route may be at most twice as far from it as the unfused one -- the bound
    tests/test_gpu_classifier.py:86 (`assert ef <= 2 * eu`) holds its fused readout to against its unfused route"""
    model, fused, unfused = make_pair(dev, n, seed=B + n + L)
    ids, pos = draw_batch(dev, B, L, seed=L + B)
    label_pos = pos[pos >= 1]

    def run(m, autocast):
        m.zero_grad(set_to_none=True)
        with torch.autocast(dev.type, dtype=dtype, enabled=autocast):
            logits = m(ids)
            loss = m.loss(ids, label_pos)
        loss.backward()
        return logits.float().detach(), m.soft_tokens.grad.clone()
    ref = run(unfused, False)
    f, u = run(fused, True), run(unfused, True)
    for name, r, a_, b_ in zip(("logits", "soft_tokens.grad"), ref, f, u):
        ef, eu = _rel(a_, r), _rel(b_, r)
        print(f"[soft-prompt autocast] B={B} n={n} L={L} {name}: fused {ef:.3e} unfused {eu:.3e}", flush=True)
        assert bool(torch.isfinite(a_).all()) and ef <= 2 * eu, (name, ef, eu)


def check_dropouts_repeat(dev, B=2, n=5, L=59):
    """both dropouts on (training mode): two calls from the same torch seed agree bit for bit, another seed does not; the soft rows' mask is the same in
    every batch row"""
    from hyena_dna_amd.block import soft_embedding_dropout_add_layer_norm
    model, fused, _ = make_pair(dev, n, seed=3, pdrop=0.5)
    fused.train()
    ids, pos = draw_batch(dev, B, L, seed=9)

    def run(seed):
        torch.manual_seed(seed)
        fused.zero_grad(set_to_none=True)
        logits = fused(ids)
        logits.float().square().mean().backward()
        return logits.detach().clone(), fused.soft_tokens.grad.clone()
    a_, b_, c_ = run(5), run(5), run(6)
    assert torch.equal(a_[0], b_[0]) and torch.equal(a_[1], b_[1]), "the same seed gave other bits"
    assert not torch.equal(a_[0], c_[0]), "another seed gave the same logits"
    blk0 = model.backbone.layers[0]
    torch.manual_seed(1)
    _, res = soft_embedding_dropout_add_layer_norm(ids, model.backbone.embeddings.word_embeddings.weight, fused.soft_tokens.detach(), blk0.norm1.weight,
                                                   blk0.norm1.bias, 0.0, 0.5, blk0.norm1.eps)
    soft_rows = res.view(B, n + L, 64)[:, :n]
    assert all(torch.equal(soft_rows[0], soft_rows[b]) for b in range(B)), "the soft tokens' mask differs between batch rows"
    dropped = soft_rows[0] == 0
    assert bool(dropped.any()) and bool((~dropped).any())
    assert torch.equal(soft_rows[0][~dropped], (fused.soft_tokens.detach() * f32(2.0))[~dropped])


def check_tuning_moves_only_the_prompt(dev, B=2, n=5, L=59, steps=20):
    model, fused, _ = make_pair(dev, n, seed=4)
    ids, pos = draw_batch(dev, B, L, seed=2)
    label_pos = pos[pos >= 1]
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    opt = torch.optim.AdamW([fused.soft_tokens], lr=3e-2, weight_decay=0.0)
    losses = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = fused.loss(ids, label_pos)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    final = fused.loss(ids, label_pos).item()
    print(f"[soft-prompt tuning] loss {losses[0]:.4f} -> {final:.4f}", flush=True)
    assert final < losses[0], (losses[0], final)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k + " moved"
    assert [nme for nme, p in fused.named_parameters() if p.requires_grad] == ["soft_tokens"]


def check_limits_and_plain_model(dev):
    from hyena_dna_amd.soft_prompt import SoftPromptLM
    model, fused, unfused = make_pair(dev, 5, seed=6)
    ids, _ = draw_batch(dev, 2, L_MAX - 4, seed=1)                    # 5 + 126 = 131 > l_max = 130
    for m in (fused, unfused):
        try:
            m(ids)
        except ValueError as e:
            assert "l_max" in str(e)
        else:
            raise AssertionError("n + L > l_max did not raise")
    plain = SoftPromptLM(model, 0).eval()
    assert plain.soft_tokens is None and not list(plain.parameters(recurse=False))
    ids, pos = draw_batch(dev, 2, 59, seed=1)
    with torch.no_grad():
        want = model(ids)[0].logits
        assert torch.equal(plain(ids), want)
        at = plain(ids, pos)
        assert bool(((at.double() - want[:, pos].double()).abs() <= _head_bound(model.hidden_at(ids, pos), model.lm_head.weight)).all())
        assert torch.equal(plain.predict(ids), want[:, -1].argmax(-1))
        assert torch.equal(fused.predict(ids), fused(ids)[:, -1].argmax(-1))


def check_padding(dev, monkeypatch, B=2, n=5, L=122):
    """an odd total n + L = 127: the padded run (128 positions) against the run as it comes, at the bounds of tests/test_lm_padding_emu.py
    test_padded_batch_equals_unpadded_batch (logits 2e-5, gradients 2e-4 relative L2)"""
    import hyena_dna_amd.lm as LM
    from tests.lm_golden import mixer_lengths
    model, fused, unfused = make_pair(dev, n, seed=8)
    ids, pos = draw_batch(dev, B, L, seed=3)
    res = {}
    for pad in (True, False):
        monkeypatch.setattr(LM, "PAD_SEQUENCES", pad)
        for name, m in (("fused", fused), ("unfused", unfused)):
            m.zero_grad(set_to_none=True)
            with mixer_lengths(model) as seen:
                logits = m(ids)
            assert seen == [128 if pad else 127] * 2 and logits.shape == (B, L, 16)
            logits.float().square().mean().backward()
            res[pad, name] = (logits.detach().clone(), m.soft_tokens.grad.clone())
    for name in ("fused", "unfused"):
        assert _rel(res[True, name][0], res[False, name][0]) < 2e-5, name
        assert _rel(res[True, name][1], res[False, name][1]) < 2e-4, name
    assert torch.equal(res[True, "fused"][0], res[True, "unfused"][0]) and torch.equal(res[True, "fused"][1], res[True, "unfused"][1])
