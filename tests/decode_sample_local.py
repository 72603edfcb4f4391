"""The device token sampler (csrc/decode_kernels.h decode_sample_kernel, include/hyena_decode.h hyena_decode_sample, generate(sampler="device"))
held to an fp64 restatement of its specification.  The cases live here and run twice: under tests/hipemu on the CPU (test_decode_sample_emu.py)
and on the gfx950 binary (test_gpu_decode_sample.py).

What may differ between the fp32 kernel and the fp64 restatement, and is therefore left out of the token comparison (never more than 1 % of a
case's draws -- asserted): a draw whose u Z' lies within relative 1e-5 of a cumulative boundary that separates two tokens, or -- for
top_p < 1 -- whose nucleus has a boundary within 1e-6 Z of top_p Z.  (At top_p = 1 the nucleus test reads "mass before < Z": it can only fail
for trailing tokens whose mass fp32 absorbs, below 64 * 2^-24 Z = 4e-6 Z in total; dropping them moves Z' by that relative amount, so a draw
can change only where u Z' already lies within 1e-5 of a boundary.  Counting the 1e-6 Z rule there as well would throw out every row whose
smallest token has p < 1e-6 Z -- four in ten rows of 64 N(0, 2^2) logits at T = 0.7 -- for no difference in the outcome.)

The sampler is a total function of its logits: a NaN ranks before every number (torch's stable descending sort), and a row whose rank-0 logit is
NaN or infinite emits its rank-0 token whatever the settings -- deterministic, so such a row is never left out (section 2b, case_nonfinite)."""
import functools

import numpy as np
import torch

SEED = 0x1234_5678_9ABC_DEF1
NCOLS = 8
B_CASE = 256


def _words(seed):
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def uniforms(seed, B, ncols):
    """u[b, c] = (word 0 of Philox4x32-10(counter (c, b), key seed) >> 8) 2^-24 from the published generator, (B, ncols) float64"""
    from tests.test_block_emu import _philox4x32_10
    k0, k1 = _words(seed)
    return np.array([[(_philox4x32_10(c, b, k0, k1)[0] >> 8) * 2.0 ** -24 for c in range(ncols)] for b in range(B)], dtype=np.float64)


def seed_tensor(seed, dev):
    return torch.tensor([seed if seed < 2 ** 63 else seed - 2 ** 64], dtype=torch.int64).to(dev)


# ---- the fp64 restatement of the specification, vectorised over rows -------------------------------------------------------------------------
def reference(l, Vlive, T, top_k, top_p, u):
    """l (B, V) float64 = float(logit); T the fp32 value of the temperature as float64; u (B,) float64.
    -> tok (B,) int64, left_out (B,) bool (the draws fp32 may legitimately decide otherwise)"""
    B, V = l.shape
    j = np.arange(V)
    live = j < Vlive
    lower = j[None, None, :] < j[None, :, None]
    nan = np.isnan(l)
    gt = np.where(nan[:, None, :], ~nan[:, :, None] | lower,                     # [b, i, j]: j before i -- a NaN before every number, the lower
                  (l[:, None, :] > l[:, :, None]) | ((l[:, None, :] == l[:, :, None]) & lower))     # NaN first; numbers: greater, then lower
    r = (gt & live[None, None, :]).sum(-1)                                       # (B, V) rank of token i among the live ones
    assert (np.sort(r[:, :Vlive], 1) == j[None, :Vlive]).all()                   # a permutation, whatever the row holds
    by_rank = np.zeros((B, Vlive), dtype=np.int64)
    rows = np.arange(B)[:, None].repeat(Vlive, 1)
    by_rank[rows, r[:, :Vlive]] = j[None, :Vlive]
    if top_k <= 1:
        return by_rank[:, 0], np.zeros(B, dtype=bool)
    k = min(top_k, Vlive)
    total = ~np.isfinite(l[rows[:, 0], by_rank[:, 0]])                           # rank 0 is NaN, +inf or -inf: the row emits its rank-0 token
    if total.any():
        tok, left_out = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=bool)
        tok[total] = by_rank[total, 0]
        if not total.all():
            tok[~total], left_out[~total] = reference(l[~total], Vlive, T, top_k, top_p, u[~total])
        return tok, left_out
    ls = np.take_along_axis(l, by_rank, 1)[:, :k]                                # kept logits in rank order
    with np.errstate(invalid="ignore"):
        p = np.exp((ls - ls[:, :1]) / T)
    incl = np.cumsum(p, 1)
    Z = incl[:, -1]
    before = incl - p
    keep = before < top_p * Z[:, None]
    nk = keep.sum(1)
    assert (keep == (np.arange(k)[None] < nk[:, None])).all() and (nk >= 1).all()         # a prefix in rank order, never empty
    Zk = incl[rows[:, 0], nk - 1]
    target = u * Zk
    inner = np.arange(k)[None] < (nk - 1)[:, None]                               # the boundaries between two kept tokens
    hit = (incl > target[:, None]) & keep
    first = np.where(hit.any(1), hit.argmax(1), nk - 1)
    tok = by_rank[rows[:, 0], first]
    left_out = (inner & (np.abs(target[:, None] - incl) <= 1e-5 * incl)).any(1)
    if top_p < 1.0:
        left_out |= (np.abs(before - top_p * Z[:, None]) <= 1e-6 * Z[:, None]).any(1)
    return tok, left_out


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def make_logits(V, Vlive, dtype, seed):
    """(B_CASE, V) N(0, 2^2) logits in `dtype`; planted: every 8th row repeats its maximum at a second live column, every 16th + 1 row has a
    -inf, every 16th + 2 row is constant over a few columns (bf16 rounding repeats values on its own as well)"""
    g = torch.Generator().manual_seed(seed)
    l = (torch.randn(B_CASE, V, generator=g) * 2.0).to(dtype)
    if Vlive >= 4:
        for b in range(0, B_CASE, 8):
            i = int(l[b, :Vlive].float().argmax())
            l[b, (i + 3) % Vlive] = l[b, i]
        for b in range(1, B_CASE, 16):
            l[b, (b // 16) % Vlive] = float("-inf")
        for b in range(2, B_CASE, 16):
            l[b, 1:4] = l[b, 0]
    return l


def make_cols(seed):
    """mixed columns: most rows somewhere in [0, NCOLS), a few parked on either side"""
    g = torch.Generator().manual_seed(seed + 1)
    col = torch.randint(0, NCOLS, (B_CASE,), generator=g, dtype=torch.int32)
    col[5::37] = -1
    col[11::41] = NCOLS
    return col


def run_kernel(_lib, dev, logits, col, seed, T, top_k, top_p, Vlive, eos=-1, pad=0, done=None, want_scores=True):
    """one call on fresh, sentinel-filled outputs -> dict of CPU tensors"""
    B, V = logits.shape
    seq = torch.full((B, NCOLS), -7, dtype=torch.int64).to(dev)
    nxt = torch.full((B, 1), -9, dtype=torch.int64).to(dev)
    colv = col.clone().to(dev)
    donev = (torch.zeros(B, dtype=torch.int32) if done is None else done.clone()).to(dev)
    scores = torch.full((B, NCOLS, V), float("nan")).to(dev) if want_scores else None
    u_out = torch.full((B,), float("nan")).to(dev)
    _lib.decode_sample(logits.to(dev), seed_tensor(seed, dev), colv, donev, seq, nxt, temperature=T, top_k=top_k, top_p=top_p, eos=eos, pad=pad,
                       vocab=Vlive, scores=scores, u_out=u_out)
    return dict(seq=seq.cpu(), nxt=nxt.cpu()[:, 0], col=colv.cpu(), done=donev.cpu(), scores=None if scores is None else scores.cpu(),
                u=u_out.cpu())


# ---- 1. the generator --------------------------------------------------------------------------------------------------------------------------
def case_philox(_lib, dev):
    V = 12
    logits = torch.zeros(64, V)
    for seed in (0, 1, SEED, 2 ** 64 - 1):
        want = uniforms(seed, 64, NCOLS)
        for c in range(NCOLS):
            out = run_kernel(_lib, dev, logits, torch.full((64,), c, dtype=torch.int32), seed, 1.0, V, 1.0, V)
            assert torch.equal(out["u"].double(), torch.from_numpy(want[:, c])), (seed, c)


# ---- 2. the kernel against the restatement -------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (12, 12), (12, 8), (16, 16), (16, 12), (64, 64), (64, 60)]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def case_kernel_vs_reference(_lib, dev, V, Vlive, dtype):
    logits = make_logits(V, Vlive, dtype, 100 * V + Vlive)
    col = make_cols(V + Vlive)
    l64 = logits.double().numpy()
    livecol = (col >= 0) & (col < NCOLS)
    u_all = uniforms(SEED, B_CASE, NCOLS)
    u = u_all[np.arange(B_CASE), col.clamp(0, NCOLS - 1).numpy()]
    rows = torch.arange(B_CASE)
    for top_k in (1, 4, V):
        for top_p in (1.0, 0.9, 0.3):
            for T in (1.0, 0.7):
                T32 = float(np.float32(T))
                want, left_out = reference(l64, Vlive, T32, top_k, float(np.float32(top_p)), u)
                n_left = int((left_out & livecol.numpy()).sum())
                print(f"V={V} Vlive={Vlive} {dtype} top_k={top_k} top_p={top_p} T={T}: {n_left} of {int(livecol.sum())} draws left out")
                assert n_left <= 0.01 * int(livecol.sum())
                out = run_kernel(_lib, dev, logits, col, SEED, T, top_k, top_p, Vlive)
                cmp = livecol & ~torch.from_numpy(left_out)
                got = out["seq"][rows, col.clamp(0, NCOLS - 1).long()]
                bad = (got != torch.from_numpy(want)) & cmp
                assert not bad.any(), (top_k, top_p, T, bad.nonzero()[:4].tolist(), got[bad][:4].tolist(), want[bad.numpy()][:4].tolist())
                assert torch.equal(out["nxt"][livecol], got[livecol]) and (got[livecol] < Vlive).all() and (got[livecol] >= 0).all()
                # scores = l / T to fp32 rounding at (b, col[b]); nothing else of scores written
                s = out["scores"][rows, col.clamp(0, NCOLS - 1).long()].double()[livecol]
                ref = torch.from_numpy(l64 / T32)[livecol]
                fin = torch.isfinite(ref)
                assert torch.equal(s[~fin], ref[~fin]) and ((s[fin] - ref[fin]).abs() <= 2.0 ** -23 * ref[fin].abs()).all()
                mask = torch.zeros(B_CASE, NCOLS, dtype=torch.bool)
                mask[rows[livecol], col[livecol].long()] = True
                assert torch.isnan(out["scores"][~mask]).all()


def case_greedy_ties(_lib, dev, dtype):
    """rows with repeated maxima: greedy takes the lowest index (checked directly, not through the restatement)"""
    V = 16
    l = torch.full((B_CASE, V), -1.0)
    g = torch.Generator().manual_seed(3)
    first = torch.randint(0, V - 2, (B_CASE,), generator=g)
    for b in range(B_CASE):
        l[b, first[b]:first[b] + 1 + b % 3] = 2.5                               # one, two or three equal maxima
    out = run_kernel(_lib, dev, l.to(dtype), torch.zeros(B_CASE, dtype=torch.int32), SEED, 1.0, 1, 0.5, V)
    assert torch.equal(out["seq"][:, 0], first) and torch.isnan(out["u"]).all()  # (greedy draws nothing)


# ---- 2b. non-finite logits: the sampler is a total function ----------------------------------------------------------------------------------
NF_SHAPES = [(12, 12), (16, 12), (64, 64), (64, 60)]
NF_KINDS = ("one NaN off the maximum", "two NaNs", "all live NaN", "one +inf", "two +inf", "NaN and +inf", "all live -inf", "NaN in a dead column")
SMP_MAX_GRID = 1 << 16                                                           # csrc/decode_kernels.h: rows from there on share a workgroup with row b - 2^16


def plant_nonfinite(l, Vlive):
    """row b gets NF_KINDS[b % 8], at columns that move with b // 8; kind 7 (nothing planted where Vlive == V) must behave as a clean row"""
    l = l.clone()
    V = l.shape[1]
    nan, inf = float("nan"), float("inf")
    for b in range(l.shape[0]):
        kind, c = b % 8, (b // 8) % Vlive
        if kind == 0:
            l[b, (int(l[b, :Vlive].float().argmax()) + 1) % Vlive] = nan
        elif kind == 1:
            l[b, c], l[b, (c + 5) % Vlive] = nan, nan
        elif kind == 2:
            l[b, :Vlive] = nan
        elif kind == 3:
            l[b, (c + 2) % Vlive] = inf
        elif kind == 4:
            l[b, c], l[b, (c + 7) % Vlive] = inf, inf
        elif kind == 5:
            l[b, c], l[b, (c + (1 if (b // 8) % 2 else Vlive - 1)) % Vlive] = inf, nan      # the NaN after the +inf, or before it
        elif kind == 6:
            l[b, :Vlive] = -inf
        elif Vlive < V:
            l[b, Vlive + (b // 8) % (V - Vlive)] = nan
    return l


def _same_with_nans(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)])


def case_nonfinite(_lib, dev, V, Vlive, dtype):
    """256 rows, NF_KINDS by row index modulo 8, against the restatement: the planted rows exactly and without exception, the clean ones (kind 7)
    as in case_kernel_vs_reference and bitwise what the call without any planted row gives them"""
    base = make_logits(V, Vlive, dtype, 100 * V + Vlive)
    logits = plant_nonfinite(base, Vlive)
    col = make_cols(V + Vlive)
    l64 = logits.double().numpy()
    livecol = (col >= 0) & (col < NCOLS)
    cc = col.clamp(0, NCOLS - 1).long()
    u = uniforms(SEED, B_CASE, NCOLS)[np.arange(B_CASE), cc.numpy()]
    rows = torch.arange(B_CASE)
    clean = rows % 8 == 7
    # the restatement's order is torch's: stable descending sort, and greedy is torch.argmax
    order = torch.sort(logits[:, :Vlive], descending=True, stable=True, dim=1).indices
    greedy, _ = reference(l64, Vlive, 1.0, 1, 1.0, u)
    assert torch.equal(torch.from_numpy(greedy), order[:, 0]) and torch.equal(order[:, 0], torch.argmax(logits[:, :Vlive], dim=1))
    eos = 3
    for top_k in (1, 4, Vlive):
        for top_p in (1.0, 0.3):
            for T in (1.0, 0.7):
                T32 = float(np.float32(T))
                want, left_out = reference(l64, Vlive, T32, top_k, float(np.float32(top_p)), u)
                assert not (left_out & ~clean.numpy()).any()                     # planted rows are deterministic: none may be left out
                top = torch.from_numpy(l64)[rows, order[:, 0]]
                assert bool((torch.from_numpy(want)[~torch.isfinite(top)] == order[:, 0][~torch.isfinite(top)]).all())
                assert not torch.isfinite(top[rows % 8 < 7]).any() and torch.isfinite(top[clean]).all()
                n_left, n_clean = int((left_out & livecol.numpy()).sum()), int((livecol & clean).sum())
                print(f"V={V} Vlive={Vlive} {dtype} top_k={top_k} top_p={top_p} T={T}: {n_left} of {n_clean} clean draws left out")
                assert n_left <= 0.01 * n_clean
                out = run_kernel(_lib, dev, logits, col, SEED, T, top_k, top_p, Vlive, eos=eos)
                got = out["seq"][rows, cc]
                assert bool(((got >= 0) & (got < Vlive))[livecol].all()), got[livecol & ((got < 0) | (got >= Vlive))][:8].tolist()
                bad = (got != torch.from_numpy(want)) & livecol & ~torch.from_numpy(left_out)
                assert not bad.any(), (top_k, top_p, T, bad.nonzero()[:8, 0].tolist(), got[bad][:8].tolist(), want[bad.numpy()][:8].tolist())
                # the sentinel rules: one element of seq per live row, next the same, col + 1, done on eos, u drawn unless greedy, scores = l / T
                assert torch.equal(out["nxt"][livecol], got[livecol]) and bool((out["nxt"][~livecol] == -9).all())
                changed = out["seq"] != -7
                assert torch.equal(changed.sum(1), livecol.long()) and bool(changed[rows[livecol], cc[livecol]].all())
                assert torch.equal(out["col"], col + livecol.int()) and torch.equal(out["done"], (livecol & (got == eos)).int())
                if top_k <= 1:
                    assert torch.isnan(out["u"]).all()
                else:
                    assert torch.equal(out["u"][livecol].double(), torch.from_numpy(u)[livecol]) and torch.isnan(out["u"][~livecol]).all()
                s = out["scores"][rows, cc].double()[livecol]
                ref = torch.from_numpy(l64 / T32)[livecol]
                fin = torch.isfinite(ref)
                assert _same_with_nans(s[~fin], ref[~fin]) and ((s[fin] - ref[fin]).abs() <= 2.0 ** -23 * ref[fin].abs()).all()
                mask = torch.zeros(B_CASE, NCOLS, dtype=torch.bool)
                mask[rows[livecol], cc[livecol]] = True
                assert torch.isnan(out["scores"][~mask]).all()
                # the clean rows among planted ones, and with a NaN in a dead column: the bits of the call that holds no planted row
                alone = run_kernel(_lib, dev, base, col, SEED, T, top_k, top_p, Vlive, eos=eos, want_scores=False)
                assert torch.equal(alone["seq"][clean], out["seq"][clean]) and torch.equal(alone["done"][clean], out["done"][clean])


def case_nonfinite_grid_stride(_lib, dev, dtype):
    """B = SMP_MAX_GRID + 256: workgroup b runs planted row b, then the clean row b + 2^16 with whatever the planted row left in LDS.  The clean
    rows' tokens are those of the call in which the planted rows are parked (the draw depends on the row index, so the rows keep their places)"""
    from tests.test_block_emu import _philox4x32_10
    V, Vlive, n = 16, 12, B_CASE
    B = SMP_MAX_GRID + n
    base = make_logits(V, Vlive, dtype, 7)
    logits = torch.zeros(B, V, dtype=dtype)
    logits[:n] = plant_nonfinite(base, Vlive)
    logits[SMP_MAX_GRID:] = base
    head, tail = slice(0, n), slice(SMP_MAX_GRID, B)
    col = torch.full((B,), -1, dtype=torch.int32)                               # rows n .. 2^16 - 1 stay parked
    col[tail] = 2
    col_planted = col.clone()
    col_planted[head] = 5
    k0, k1 = _words(SEED)
    u_head = np.array([(_philox4x32_10(5, b, k0, k1)[0] >> 8) * 2.0 ** -24 for b in range(n)])
    u_tail = np.array([(_philox4x32_10(2, b, k0, k1)[0] >> 8) * 2.0 ** -24 for b in range(SMP_MAX_GRID, B)])
    for top_k, top_p in ((1, 1.0), (4, 0.3), (Vlive, 1.0)):
        T32 = float(np.float32(0.7))
        want_h, left_h = reference(logits[head].double().numpy(), Vlive, T32, top_k, float(np.float32(top_p)), u_head)
        want_t, left_t = reference(logits[tail].double().numpy(), Vlive, T32, top_k, float(np.float32(top_p)), u_tail)
        planted = np.arange(n) % 8 < 7
        assert not left_h[planted].any() and int(left_t.sum()) <= 0.01 * n
        alone = run_kernel(_lib, dev, logits, col, SEED, 0.7, top_k, top_p, Vlive, want_scores=False)
        both = run_kernel(_lib, dev, logits, col_planted, SEED, 0.7, top_k, top_p, Vlive, want_scores=False)
        assert bool((alone["seq"][:SMP_MAX_GRID] == -7).all()) and bool((both["seq"][n:SMP_MAX_GRID] == -7).all())
        assert torch.equal(both["seq"][tail], alone["seq"][tail]) and torch.equal(both["nxt"][tail], alone["nxt"][tail])
        got_t, got_h = both["seq"][tail, 2], both["seq"][head, 5]
        assert bool(((got_t >= 0) & (got_t < Vlive)).all()) and bool(((got_h >= 0) & (got_h < Vlive)).all())
        assert torch.equal(got_t[~left_t], torch.from_numpy(want_t)[~left_t]), (top_k, top_p)
        assert torch.equal(got_h[planted], torch.from_numpy(want_h)[planted]), (top_k, top_p)


# ---- 3. the distribution of the draws ----------------------------------------------------------------------------------------------------------
def case_distribution(_lib, dev):
    V, B = 12, 1024
    row = torch.tensor([1.5, -0.3, 0.2, 2.1, -1.7, 0.9, 0.0, -0.6, 1.1, -2.4, 0.5, 1.8])
    p = torch.softmax(row.double() / float(np.float32(0.9)), 0)
    logits = row[None].repeat(B, 1).to(dev)
    seq = torch.full((B, NCOLS), -1, dtype=torch.int64).to(dev)
    nxt = torch.zeros(B, 1, dtype=torch.int64).to(dev)
    col, done = torch.zeros(B, dtype=torch.int32).to(dev), torch.zeros(B, dtype=torch.int32).to(dev)
    seed = seed_tensor(SEED, dev)
    for _ in range(NCOLS):
        _lib.decode_sample(logits, seed, col, done, seq, nxt, temperature=0.9, top_k=V, top_p=1.0)
    assert col.cpu().tolist() == [NCOLS] * B
    n = B * NCOLS
    freq = torch.bincount(seq.cpu().reshape(-1), minlength=V).double() / n
    bound = 4 * torch.sqrt(p * (1 - p) / n)
    print("frequency - p, in units of the bound:", ((freq - p) / bound).tolist())
    assert ((freq - p).abs() <= bound).all()


# ---- 4. state ------------------------------------------------------------------------------------------------------------------------------------
def case_state(_lib, dev):
    V, B = 12, 6
    g = torch.Generator().manual_seed(9)
    logits = torch.randn(B, V, generator=g) * 2
    logits[4] = -5.0
    logits[4, 7] = 9.0                                                          # row 4 draws token 7 = eos (its mass is 1 to fp32)
    col = torch.tensor([0, -1, NCOLS, 3, 5, NCOLS - 1], dtype=torch.int32)      # rows 1, 2 parked
    done = torch.tensor([0, 0, 0, 1, 0, 0], dtype=torch.int32)                  # row 3 finished
    out = run_kernel(_lib, dev, logits, col, SEED, 1.0, 4, 0.9, V, eos=7, pad=11, done=done)
    assert out["col"].tolist() == [1, -1, NCOLS, 3, 6, NCOLS]                   # live rows advance by one, the others stay
    assert out["nxt"][1] == -9 and out["nxt"][2] == -9 and out["nxt"][3] == 11  # parked: untouched; done: pad
    assert out["seq"][4, 5] == 7 and out["done"].tolist()[1:5] == [0, 0, 1, 1]    # an EOS draw sets done; parked and done rows keep theirs
    assert out["done"][0] == int(out["seq"][0, 0] == 7) and out["done"][5] == int(out["seq"][5, NCOLS - 1] == 7)
    changed = out["seq"] != -7
    assert changed.sum(1).tolist() == [1, 0, 0, 0, 1, 1]                        # exactly one element per live row
    assert changed[0, 0] and changed[4, 5] and changed[5, NCOLS - 1]
    for b in (1, 2, 3):
        assert torch.isnan(out["scores"][b]).all() and torch.isnan(out["u"][b])
    for b in (0, 4, 5):
        assert not torch.isnan(out["u"][b]) and torch.isnan(out["scores"][b]).sum() == (NCOLS - 1) * V
        assert out["nxt"][b] == out["seq"][b, col[b]]


# ---- 5. refusals: HYENA_ERR_BAD_ARG before anything is launched ----------------------------------------------------------------------------------
def case_refusals(_lib, dev):
    import ctypes
    L = _lib.lib()
    B, V, ncols = 2, 16, 8
    t = dict(logits=torch.zeros(B, V), seed=torch.zeros(1, dtype=torch.int64), col=torch.zeros(B, dtype=torch.int32),
             done=torch.zeros(B, dtype=torch.int32), seq=torch.zeros(B, ncols, dtype=torch.int64), nxt=torch.zeros(B, dtype=torch.int64))
    t = {k: v.to(dev) for k, v in t.items()}

    def call(**kw):
        a = dict(logits=t["logits"].data_ptr(), ldl=V, dtype=0, B=B, V=V, Vlive=12, T=1.0, top_k=4, top_p=0.9, seed=t["seed"].data_ptr(), eos=-1,
                 pad=0, col=t["col"].data_ptr(), done=t["done"].data_ptr(), seq=t["seq"].data_ptr(), lds=ncols, ncols=ncols, nxt=t["nxt"].data_ptr(),
                 ldn=1)
        a.update(kw)
        return L.hyena_decode_sample(a["logits"], a["ldl"], a["dtype"], a["B"], a["V"], a["Vlive"], ctypes.c_float(a["T"]), a["top_k"],
                                     ctypes.c_float(a["top_p"]), a["seed"], a["eos"], a["pad"], a["col"], a["done"], a["seq"], a["lds"],
                                     a["ncols"], a["nxt"], a["ldn"], None, None, None)

    for name in ("logits", "seed", "col", "done", "seq", "nxt"):
        assert call(**{name: None}) == 1, name
    for kw in (dict(V=65, ldl=65), dict(Vlive=0), dict(Vlive=17), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=-0.1), dict(top_p=float("nan")),
               dict(dtype=3), dict(dtype=-1), dict(ldl=V - 1), dict(lds=ncols - 1)):
        assert call(**kw) == 1, kw
    assert (t["seq"] == 0).all() and (t["col"] == 0).all()                      # nothing ran
    if dev == "cpu":                                                            # (the emulation: the good call really runs)
        assert call() == 0 and t["col"].tolist() == [1, 1]


# ---- 6. the language model ---------------------------------------------------------------------------------------------------------------------
def tiny_lm(dev, vocab=12, n_layer=2, L=256, seed=0):
    from hyena_dna_amd.lm import HyenaDNALM
    torch.manual_seed(seed)
    layer = dict(l_max=L, order=2, filter_order=64, emb_dim=5, short_filter_order=3, modulate=True, w=10, lr=6e-4, wd=0.0, lr_pos_emb=0.0)
    m = HyenaDNALM(d_model=64, n_layer=n_layer, d_inner=256, vocab_size=vocab, layer=layer, resid_dropout=0.0, embed_dropout=0.1,
                   pad_vocab_size_multiple=8, fused_dropout_add_ln=True, residual_in_fp32=True)
    return m.to(dev).eval()


B_LM, P_LM, N_LM, PAD = 3, 10, 24, 4
LENS = (10, 6, 1)


def lm_inputs(dev):
    ids = torch.randint(7, 11, (B_LM, P_LM), generator=torch.Generator().manual_seed(2)).to(dev)
    return ids, torch.tensor(LENS, dtype=torch.int32).to(dev)


def _gen(m, ids, lengths=None, **kw):
    kw.setdefault("use_cache", True)
    return m.generate(ids, max_length=P_LM + N_LM, lengths=lengths, pad_token_id=PAD, return_dict_in_generate=True, output_scores=True, **kw)


def _new_tokens(out, lengths):
    """(B, N) the new tokens of every row"""
    start = torch.full((B_LM,), P_LM, dtype=torch.int64) if lengths is None else lengths.cpu().long()
    return out.sequences.cpu().gather(1, start[:, None] + torch.arange(N_LM))


def case_lm_greedy(dev, ragged):
    m = tiny_lm(dev)
    ids, lengths = lm_inputs(dev)
    lengths = lengths if ragged else None
    ref = _gen(m, ids, lengths, sampler="torch")
    out = _gen(m, ids, lengths, sampler="device", top_k=1)
    assert torch.equal(out.sequences, ref.sequences) and out.sequences.dtype == torch.int64 and out.sequences.shape == (B_LM, P_LM + N_LM)
    assert len(out.scores) == N_LM and out.scores[0].shape == (B_LM, 16) and out.scores[0].dtype == torch.float32
    for a, b in zip(out.scores, ref.scores):
        assert torch.equal(a, b.float())                                        # (T = 1: l / T is l)
    if ragged:
        assert torch.equal(out.lengths, lengths + N_LM) and out.lengths.dtype == torch.int32
    toks = _new_tokens(out, lengths)
    for i, s in enumerate(out.scores):                                          # every emitted token attains the maximum of its scores row
        s = s.cpu()
        assert torch.equal(s[torch.arange(B_LM), toks[:, i]], s.max(-1).values), i
    # top_p -> 0 keeps the top-ranked token alone: greedy whatever the seed; plain sequences are returned without the dict
    seq = m.generate(ids, max_length=P_LM + N_LM, lengths=lengths, pad_token_id=PAD, use_cache=True, top_k=4, top_p=1e-6, seed=5)
    assert torch.equal(seq, ref.sequences)


def case_lm_seeded(dev, ragged):
    m = tiny_lm(dev)
    ids, lengths = lm_inputs(dev)
    lengths = lengths if ragged else None
    kw = dict(top_k=4, top_p=0.9, temperature=1.3)
    a, b, c = _gen(m, ids, lengths, seed=11, **kw), _gen(m, ids, lengths, seed=11, **kw), _gen(m, ids, lengths, seed=12, **kw)
    assert torch.equal(a.sequences, b.sequences) and all(torch.equal(x, y) for x, y in zip(a.scores, b.scores))
    assert not torch.equal(a.sequences, c.sequences)
    torch.manual_seed(0)
    d = _gen(m, ids, lengths, top_p=0.9, top_k=4, temperature=1.3)             # seed=None: from torch's generator, once per call
    torch.manual_seed(0)
    e = _gen(m, ids, lengths, top_p=0.9, top_k=4, temperature=1.3)
    assert torch.equal(d.sequences, e.sequences)
    # the padded vocabulary
    wide = dict(top_k=16, temperature=50.0, seed=3)                             # nearly uniform over what is allowed
    assert (_new_tokens(_gen(m, ids, lengths, **wide), lengths) >= 12).any()
    assert (_new_tokens(_gen(m, ids, lengths, vocab_size=12, **wide), lengths) < 12).all()


def case_lm_eos(dev, ragged):
    m = tiny_lm(dev)
    ids, lengths = lm_inputs(dev)
    lengths = lengths if ragged else None
    kw = dict(top_k=4, temperature=1.5, seed=21, vocab_size=12)
    free = _gen(m, ids, lengths, **kw)
    toks = _new_tokens(free, lengths)
    # the token whose first appearance, taken over the rows, comes earliest last: every row finishes on it, at different steps
    cands = [t for t in toks.unique().tolist() if all((toks[b] == t).any() for b in range(B_LM)) and t != PAD]
    assert cands, toks
    firsts = {t: [int((toks[b] == t).nonzero()[0]) for b in range(B_LM)] for t in cands}
    eos = min(cands, key=lambda t: max(firsts[t]))
    first = firsts[eos]
    assert max(first) < N_LM - 2 and len(set(first)) > 1, (eos, first)
    out = _gen(m, ids, lengths, eos_token_id=eos, **kw)
    got = _new_tokens(out, lengths)
    for b in range(B_LM):
        n = first[b] + 1
        assert torch.equal(got[b, :n], toks[b, :n]) and got[b, n - 1] == eos    # the same draws up to its own EOS ...
        assert (got[b, n:] == PAD).all()                                        # ... then padding, while the slower rows go on
    assert len(out.scores) == N_LM
    early = _gen(m, ids, lengths, eos_token_id=eos, stop_check_every=1, **kw)
    assert torch.equal(early.sequences, out.sequences)
    assert len(early.scores) == max(first) + 1
    for x, y in zip(early.scores, out.scores):
        assert torch.equal(x, y)
    assert len(_gen(m, ids, lengths, eos_token_id=eos, stop_check_every=5, **kw).scores) == min(N_LM, -(-(max(first) + 1) // 5) * 5)


def case_lm_refusals(dev):
    import pytest
    m = tiny_lm(dev, n_layer=1)
    ids, lengths = lm_inputs(dev)
    with pytest.raises(ValueError, match="use_cache=True"):
        m.generate(ids, max_length=14, sampler="device")
    with pytest.raises(ValueError, match="use_cache=True"):
        m.generate(ids, max_length=14, seed=3)
    for bad in (0.0, 1.5, -1.0):
        with pytest.raises(ValueError, match="top_p"):
            m.generate(ids, max_length=14, use_cache=True, top_p=bad)
    with pytest.raises(ValueError, match="sampler"):
        m.generate(ids, max_length=14, use_cache=True, sampler="host")
    with pytest.raises(ValueError, match="sampler='device'"):
        m.generate(ids, max_length=14, use_cache=True, sampler="torch", seed=3)
    with pytest.raises(ValueError, match="vocab_size"):
        m.generate(ids, max_length=14, use_cache=True, vocab_size=17)
    with pytest.raises(ValueError, match="int32"):
        m.generate(ids, max_length=14, use_cache=True, seed=1, lengths=lengths.long())
    big = tiny_lm(dev, vocab=70, n_layer=1)
    with pytest.raises(ValueError, match="at most 64 columns"):
        big.generate(ids, max_length=14, use_cache=True, seed=1)
