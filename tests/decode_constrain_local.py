"""The constrained device sampler (csrc/decode_kernels.h decode_sample_con_kernel, include/hyena_decode.h hyena_decode_sample_constrained,
generate(allowed_tokens= / constraints= / min_new_tokens= / output_logprobs=)) held to fp64 restatements of its specification.  The cases live
here and run twice: under tests/hipemu on the CPU (test_decode_constrain_emu.py) and on the gfx950 binary (test_gpu_decode_constrain.py).

Tokens.  The reference is tests/decode_sample_local.reference applied to the row's allowed columns compacted in index order (compaction keeps
the index tie-break) and mapped back.  Draws are left out of the comparison by that module's rule alone -- u Z' within 1e-5 of a cumulative
boundary, or a nucleus boundary within 1e-6 Z -- and never more than 1 % of a case's draws (asserted).

Log-probs.  The kernel computes, in fp32 (unit roundoff e = 2^-24, one ulp <= 2 e relative), with n = Vlive,
    d_j = fl(l_j - m);  S = the serial sum of expf(d_j), j = 0 .. n - 1;  lp = fl(fl(l_tok - m) - logf(S)),   m = max_j l_j.
Against lp* = (l_tok - m) - log S* in exact arithmetic (S* = sum exp(l_j - m), 1 <= S* <= n):
  * d_j carries a relative error e, so exp(d_j) a relative error |d_j| e; weighted by exp(d_j) / S* the terms |d_j| exp(d_j) <= 1 / e_euler
    each and S* >= 1, so this moves S by at most (n / 2.718) e relatively;
  * expf: no accuracy figure for the device library's expf / logf is documented under the ROCm tree of this toolchain, so 2 ulp each is
    assumed: 4 e relative on every term, hence on S;
  * a serial sum of n non-negative terms: (n - 1) e relative;
  * log of a value with relative error r moves by r (to first order): (n / 2.718 + 4 + n - 1) e absolute; logf itself 2 ulp: 4 e |log S*|;
  * fl(l_tok - m): e |l_tok - m|;  the last subtraction: e |lp*|.
BOUND = 1.01 e (n / 2.718 + n + 3 + 4 |log S*| + |l_tok - m| + |lp*|) + 2^-100 (1 % for the second-order terms, 2^-100 for masses that
underflow).  Non-finite rows are compared exactly: NaN where m or S* is not finite, -inf where only l_tok is."""
import numpy as np
import torch

from tests import decode_sample_local as DS

SEED, NCOLS, B_CASE = DS.SEED, DS.NCOLS, DS.B_CASE
SHAPES = [(12, 12), (12, 8), (16, 16), (16, 12), (64, 64), (64, 60)]
DTYPES = DS.DTYPES
FAMILIES = ("random", "acgt", "onebit", "ones", "no_argmax", "nonfinite_only", "empty_below_vlive", "outside_nallow", "mixed_start")
DS_MASK_ACGT = 0xF << 7                                                          # bits 7 .. 10: A C G T of the character tokenizer
COL = 3                                                                          # every row of a token case stands at this column
NALLOW = 4
E32 = 2.0 ** -24


def masks_to_tensor(m):
    return torch.from_numpy(np.asarray(m, dtype=np.uint64).view(np.int64).copy())


def bits(m, V):
    """uint64 array (...) -> bool (..., V)"""
    return ((np.asarray(m, dtype=np.uint64)[..., None] >> np.arange(V, dtype=np.uint64)) & np.uint64(1)).astype(bool)


def run_kernel(_lib, dev, logits, col, seed, T, top_k, top_p, Vlive, eos=-1, pad=0, done=None, allow=None, start=None, want_logprobs=False,
               ldp=NCOLS, old=False):
    """one call on fresh, sentinel-filled outputs -> dict of CPU tensors; ``old``: through hyena_decode_sample"""
    B, V = logits.shape
    seq = torch.full((B, NCOLS), -7, dtype=torch.int64).to(dev)
    nxt = torch.full((B, 1), -9, dtype=torch.int64).to(dev)
    colv = col.clone().to(dev)
    donev = (torch.zeros(B, dtype=torch.int32) if done is None else done.clone()).to(dev)
    scores = torch.full((B, NCOLS, V), float("nan")).to(dev)
    u_out = torch.full((B,), float("nan")).to(dev)
    lp = torch.full((B, ldp), -777.0).to(dev) if want_logprobs else None
    kw = {} if old else dict(allow=None if allow is None else allow.to(dev),
                             start=(torch.zeros(B, dtype=torch.int32) if start is None else start).to(dev), logprobs=lp)
    _lib.decode_sample(logits.to(dev), DS.seed_tensor(seed, dev), colv, donev, seq, nxt, temperature=T, top_k=top_k, top_p=top_p, eos=eos,
                       pad=pad, vocab=Vlive, scores=scores, u_out=u_out, **kw)
    return dict(seq=seq.cpu(), nxt=nxt.cpu()[:, 0], col=colv.cpu(), done=donev.cpu(), scores=scores.cpu(), u=u_out.cpu(),
                lp=None if lp is None else lp.cpu())


def same_bits(a, b):
    for k in ("seq", "nxt", "col", "done"):
        assert torch.equal(a[k], b[k]), k
    for k in ("scores", "u"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


# ---- the fp64 restatement ------------------------------------------------------------------------------------------------------------------------
def allowed_sets(allow, start, col, Vlive, V):
    """allow None | uint64 (nallow,) | (B, nallow); start, col (B,) -> bool (B, V): the specification's A, with its three fall-backs"""
    B = len(col)
    live = np.arange(V) < Vlive
    A = np.tile(live, (B, 1))
    if allow is None:
        return A
    n = col.astype(np.int64) - start.astype(np.int64)
    nallow = allow.shape[-1]
    inside = (n >= 0) & (n < nallow)
    nn = np.clip(n, 0, nallow - 1)
    m = allow[nn] if allow.ndim == 1 else allow[np.arange(B), nn]
    mb = bits(m, V) & live[None]
    use = inside & mb.any(1)
    A[use] = mb[use]
    return A


def reference(l64, A, Vlive, T, top_k, top_p, u):
    """DS.reference on every row's allowed columns compacted in index order, mapped back -> tok (B,), left_out (B,)"""
    B, V = l64.shape
    tok, left = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=bool)
    cnt = A.sum(1)
    for nA in np.unique(cnt):
        rows = np.nonzero(cnt == nA)[0]
        idx = np.argsort(~A[rows], axis=1, kind="stable")[:, :nA]              # the allowed columns, ascending
        t, lo = DS.reference(np.take_along_axis(l64[rows], idx, 1), int(nA), T, top_k, top_p, u[rows])
        tok[rows], left[rows] = idx[np.arange(len(rows)), t], lo
    return tok, left


def logprob_reference(l64, Vlive, tok):
    """-> lp* (B,) float64 (NaN / -inf by the specification's rules), BOUND (B,)"""
    l = l64[:, :Vlive]
    B = len(l)
    lp, bound = np.full(B, np.nan), np.zeros(B)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.where(np.isnan(l), -np.inf, l).max(1)                           # fmaxf skips NaNs
        ok = np.isfinite(m) & ~np.isnan(l).any(1)
        d = l[ok] - m[ok, None]
        S = np.exp(d).sum(1)
        lt = l[ok, tok[ok]] - m[ok]
        lp[ok] = lt - np.log(S)
        fin = np.isfinite(lt)
        b = 1.01 * E32 * (Vlive / np.e + Vlive + 3 + 4 * np.abs(np.log(S)) + np.abs(np.where(fin, lt, 0.0)) + np.abs(np.where(fin, lp[ok], 0.0)))
        bound[ok] = b + 2.0 ** -100
    return lp, bound


def check_logprobs(got, want, bound, what=""):
    """got fp32 tensor, want / bound float64 arrays -> the worst |got - want| / bound over the finite ones; the others must agree exactly"""
    got = got.double().numpy()
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, np.nonzero(np.isnan(got) != np.isnan(want))[0][:8].tolist())
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), what
    if not fin.any():
        return 0.0
    ratio = np.abs(got[fin] - want[fin]) / bound[fin]
    assert (ratio <= 1.0).all(), (what, float(ratio.max()))
    return float(ratio.max())


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------------
def make_family(name, V, Vlive, dtype):
    """-> logits (B_CASE, V), allow uint64 array or None, start int32 (B_CASE,) -- every row stands at column COL"""
    logits = DS.make_logits(V, Vlive, dtype, 100 + V + Vlive)
    rng = np.random.default_rng(7 + V)
    B = B_CASE
    start = np.zeros(B, dtype=np.int32)                                        # n = COL: the last of NALLOW masks
    rand = rng.integers(0, 2 ** 64, size=(B, NALLOW), dtype=np.uint64)
    lf = logits.float()
    if name == "random":
        allow = rand
    elif name == "acgt":
        allow = np.full(NALLOW, 0xF << 7, dtype=np.uint64)                     # lda = 0; at Vlive = 8 only bit 7 is live
    elif name == "onebit":
        allow = np.uint64(1) << rng.integers(0, Vlive, size=(B, NALLOW)).astype(np.uint64)
    elif name == "ones":
        allow = np.full((B, NALLOW), 2 ** 64 - 1, dtype=np.uint64)
    elif name == "no_argmax":
        top = lf[:, :Vlive].argmax(1).numpy().astype(np.uint64)
        allow = np.repeat((~(np.uint64(1) << top))[:, None], NALLOW, 1)
    elif name == "nonfinite_only":                                              # two allowed columns per row, both -inf, both NaN, or one of each
        a, b = rng.integers(0, Vlive, size=B), rng.integers(0, Vlive, size=B)
        allow = np.repeat(((np.uint64(1) << a.astype(np.uint64)) | (np.uint64(1) << b.astype(np.uint64)))[:, None], NALLOW, 1)
        for r in range(B):
            logits[r, a[r]] = float("nan") if r % 3 == 1 else float("-inf")
            logits[r, b[r]] = float("nan") if r % 3 else float("-inf")
    elif name == "empty_below_vlive":                                           # nothing below Vlive: rows 0 mod 2 only dead bits, the others no bit
        dead = np.uint64(((1 << V) - 1) & ~((1 << Vlive) - 1) | (1 << 63 if Vlive < 64 else 0))
        allow = np.where((np.arange(B) % 2 == 0)[:, None], dead, np.uint64(0)) * np.ones((B, NALLOW), dtype=np.uint64)
    elif name == "outside_nallow":                                              # one-bit masks that must NOT apply: n = -1, or n = NALLOW
        allow = np.uint64(1) << rng.integers(0, Vlive, size=(B, NALLOW - 1)).astype(np.uint64)
        start = np.where(np.arange(B) % 2 == 0, COL + 1, 0).astype(np.int32)
        start[::5] = COL - 1                                                    # ... and every fifth row inside, n = 1
    elif name == "mixed_start":
        allow = rand
        start = rng.integers(0, COL + 1, size=B).astype(np.int32)              # n = COL - start in 0 .. COL
    else:
        raise KeyError(name)
    return logits, allow, torch.from_numpy(start)


# ---- 1. tokens against the restatement -----------------------------------------------------------------------------------------------------------
def case_tokens(_lib, dev, V, Vlive, dtype, family):
    logits, allow, start = make_family(family, V, Vlive, dtype)
    col = torch.full((B_CASE,), COL, dtype=torch.int32)
    l64 = logits.double().numpy()
    A = allowed_sets(allow, start.numpy(), col.numpy(), Vlive, V)
    if family in ("ones", "empty_below_vlive"):
        assert (A == (np.arange(V) < Vlive)[None]).all()
    if family == "outside_nallow":
        assert (A.sum(1)[::5] == 1).all() and (np.delete(A.sum(1), np.arange(0, B_CASE, 5)) == Vlive).all()
    u = DS.uniforms(SEED, B_CASE, NCOLS)[:, COL]
    at = masks_to_tensor(allow)
    eos = 8
    for top_k in (1, 4, V):
        for top_p in (1.0, 0.9, 0.3):
            for T in (1.0, 0.7):
                want, left_out = reference(l64, A, Vlive, float(np.float32(T)), top_k, float(np.float32(top_p)), u)
                n_left = int(left_out.sum())
                print(f"{family} V={V} Vlive={Vlive} {dtype} top_k={top_k} top_p={top_p} T={T}: {n_left} of {B_CASE} draws left out")
                assert n_left <= 0.01 * B_CASE
                out = run_kernel(_lib, dev, logits, col, SEED, T, top_k, top_p, Vlive, eos=eos, allow=at, start=start)
                got = out["seq"][:, COL]
                assert bool(A[np.arange(B_CASE), got.numpy()].all())            # never a token outside A, left-out draws included
                bad = (got != torch.from_numpy(want)) & ~torch.from_numpy(left_out)
                assert not bad.any(), (top_k, top_p, T, bad.nonzero()[:4, 0].tolist(), got[bad][:4].tolist(), want[bad.numpy()][:4].tolist())
                assert torch.equal(out["nxt"], got) and bool((out["col"] == COL + 1).all())
                assert torch.equal(out["done"], (got == eos).int())             # eos ends a row exactly where it was emitted
                changed = out["seq"] != -7
                assert bool((changed.sum(1) == 1).all()) and bool(changed[:, COL].all())
                if top_k > 1:
                    assert torch.equal(out["u"].double(), torch.from_numpy(u))


# ---- 2. bitwise identities -----------------------------------------------------------------------------------------------------------------------
def case_identity_with_old_kernel(_lib, dev, V, Vlive, dtype):
    """no masks / all-ones masks (per row and broadcast) against hyena_decode_sample: every output, u included; clean and non-finite rows,
    mixed, parked and done rows"""
    base = DS.make_logits(V, Vlive, dtype, 100 + V + Vlive)
    col = DS.make_cols(V + Vlive)
    done = (torch.arange(B_CASE) % 11 == 3).int()
    start = torch.zeros(B_CASE, dtype=torch.int32)
    ones_rows = torch.full((B_CASE, NCOLS), -1, dtype=torch.int64)
    ones_one = torch.full((NCOLS,), -1, dtype=torch.int64)
    for logits in (base, DS.plant_nonfinite(base, Vlive)):
        for top_k, top_p, T in ((1, 1.0, 1.0), (4, 0.9, 0.7), (V, 0.3, 1.0), (V, 1.0, 0.7)):
            kw = dict(eos=3, pad=5, done=done)
            old = run_kernel(_lib, dev, logits, col, SEED, T, top_k, top_p, Vlive, old=True, **kw)
            same_bits(old, run_kernel(_lib, dev, logits, col, SEED, T, top_k, top_p, Vlive, **kw))
            same_bits(old, run_kernel(_lib, dev, logits, col, SEED, T, top_k, top_p, Vlive, allow=ones_rows, start=start, **kw))
            with_lp = run_kernel(_lib, dev, logits, col, SEED, T, top_k, top_p, Vlive, allow=ones_one, start=start, want_logprobs=True, **kw)
            same_bits(old, with_lp)                                             # (asking for log-probs moves nothing else)


def case_forced(_lib, dev, V, Vlive, dtype):
    """a one-bit mask emits exactly that token whatever the logits are (NaN, +-inf rows included) and whatever the settings"""
    logits = DS.plant_nonfinite(DS.make_logits(V, Vlive, dtype, 100 + V + Vlive), Vlive)
    g = torch.Generator().manual_seed(V)
    want = torch.randint(0, Vlive, (B_CASE,), generator=g)
    allow = (torch.ones(B_CASE, dtype=torch.int64) << want)[:, None].repeat(1, NALLOW)      # (bit 63: 1 << 63 wraps to the sign bit)
    col = torch.full((B_CASE,), COL, dtype=torch.int32)
    for top_k, top_p, T in ((1, 1.0, 1.0), (4, 0.3, 0.7), (V, 1.0, 1.0)):
        out = run_kernel(_lib, dev, logits, col, SEED, T, top_k, top_p, Vlive, allow=allow)
        assert torch.equal(out["seq"][:, COL], want) and torch.equal(out["nxt"], want)


def case_state(_lib, dev):
    """parked and done rows write nothing beyond next = pad: seq, col, done, scores, u and the log-prob slots keep their sentinels"""
    V, B = 12, 6
    g = torch.Generator().manual_seed(9)
    logits = torch.randn(B, V, generator=g) * 2
    logits[4] = -5.0
    logits[4, 7] = 9.0
    col = torch.tensor([0, -1, NCOLS, 3, 5, NCOLS - 1], dtype=torch.int32)      # rows 1, 2 parked
    done = torch.tensor([0, 0, 0, 1, 0, 0], dtype=torch.int32)                  # row 3 finished
    start = torch.tensor([0, 0, 0, 1, 2, 4], dtype=torch.int32)
    allow = torch.full((NCOLS,), DS_MASK_ACGT, dtype=torch.int64)
    out = run_kernel(_lib, dev, logits, col, SEED, 1.0, 4, 0.9, V, eos=7, pad=11, done=done, allow=allow, start=start, want_logprobs=True)
    assert out["col"].tolist() == [1, -1, NCOLS, 3, 6, NCOLS]
    assert out["nxt"][1] == -9 and out["nxt"][2] == -9 and out["nxt"][3] == 11
    assert out["seq"][4, 5] == 7 and out["done"].tolist()[1:5] == [0, 0, 1, 1]    # eos allowed (bit 7) and emitted: the row ends
    changed = out["seq"] != -7
    assert changed.sum(1).tolist() == [1, 0, 0, 0, 1, 1]
    wrote = out["lp"] != -777.0
    assert wrote.sum(1).tolist() == [1, 0, 0, 0, 1, 1] and wrote[0, 0] and wrote[4, 3] and wrote[5, NCOLS - 1 - 4]
    for b in (1, 2, 3):
        assert torch.isnan(out["scores"][b]).all() and torch.isnan(out["u"][b])
    for b in (0, 4, 5):
        assert 7 <= out["nxt"][b] <= 10
    # eos outside the mask is never emitted and never ends a row, although it holds nearly all the mass
    out = run_kernel(_lib, dev, logits, col, SEED, 1.0, 4, 0.9, V, eos=7, pad=11, done=done, allow=allow & ~(1 << 7), start=start)
    assert 8 <= out["seq"][4, 5] <= 10 and out["done"].tolist() == [0, 0, 0, 1, 0, 0]
    # a log-prob buffer narrower than the token's number: nothing is written, the token still is
    out = run_kernel(_lib, dev, logits, col, SEED, 1.0, 4, 0.9, V, allow=allow, start=start, want_logprobs=True, ldp=3)
    assert (out["lp"] != -777.0).sum(1).tolist() == [1, 0, 0, 1, 0, 0] and out["col"].tolist() == [1, -1, NCOLS, 4, 6, NCOLS]


# ---- 3. the distribution of the draws under a mask ------------------------------------------------------------------------------------------------
def case_distribution(_lib, dev):
    V, B = 12, 1024
    row = torch.tensor([1.5, -0.3, 0.2, 2.1, -1.7, 0.9, 0.0, -0.6, 1.1, -2.4, 0.5, 1.8])
    keep = [3, 5, 8, 11]
    p = torch.zeros(V, dtype=torch.float64)
    p[keep] = torch.softmax(row.double()[keep] / float(np.float32(0.9)), 0)     # renormalised over the allowed four
    logits = row[None].repeat(B, 1).to(dev)
    seq = torch.full((B, NCOLS), -1, dtype=torch.int64).to(dev)
    nxt = torch.zeros(B, 1, dtype=torch.int64).to(dev)
    col, done = torch.zeros(B, dtype=torch.int32).to(dev), torch.zeros(B, dtype=torch.int32).to(dev)
    start = torch.zeros(B, dtype=torch.int32).to(dev)
    allow = torch.full((NCOLS,), sum(1 << v for v in keep), dtype=torch.int64).to(dev)
    seed = DS.seed_tensor(SEED, dev)
    for _ in range(NCOLS):
        _lib.decode_sample(logits, seed, col, done, seq, nxt, temperature=0.9, top_k=V, top_p=1.0, allow=allow, start=start)
    assert col.cpu().tolist() == [NCOLS] * B
    n = B * NCOLS
    freq = torch.bincount(seq.cpu().reshape(-1), minlength=V).double() / n
    bound = 4 * torch.sqrt(p * (1 - p) / n)
    print("frequency - p, in units of the bound:", ((freq - p)[keep] / bound[keep]).tolist())
    assert ((freq - p).abs() <= bound).all()                                    # (outside the mask: exactly 0 <= 0)


# ---- 4. log-probs against an fp64 log-softmax ----------------------------------------------------------------------------------------------------
def case_logprobs(_lib, dev, V, Vlive, dtype):
    base = DS.make_logits(V, Vlive, dtype, 100 + V + Vlive)
    col = DS.make_cols(V + Vlive)
    livecol = ((col >= 0) & (col < NCOLS)).numpy()
    cc = col.clamp(0, NCOLS - 1).long()
    start = torch.from_numpy(np.random.default_rng(7 + V).integers(0, 3, size=B_CASE).astype(np.int32))
    rows = torch.arange(B_CASE)
    worst = 0.0
    for name, logits in (("clean", base), ("non-finite", DS.plant_nonfinite(base, Vlive))):
        l64 = logits.double().numpy()
        for top_k, T in ((1, 1.0), (4, 0.7), (V, 1.0)):
            out = run_kernel(_lib, dev, logits, col, SEED, T, top_k, 1.0, Vlive, start=start, want_logprobs=True)
            n = (col - start).long()
            slot = torch.from_numpy(livecol) & (n >= 0) & (n < NCOLS)
            wrote = out["lp"] != -777.0
            want_wrote = torch.zeros_like(wrote)
            want_wrote[rows[slot], n[slot]] = True
            assert torch.equal(wrote, want_wrote)                               # one slot per live row with n inside the buffer, nothing else
            tok = out["seq"][rows, cc].numpy()
            lp, bound = logprob_reference(l64[slot.numpy()], Vlive, tok[slot.numpy()])
            if name == "non-finite":
                kinds = (rows % 8)[slot].numpy()                                # NaN or +inf among the live logits, or all -inf: NaN (kinds 0 .. 6)
                assert np.isnan(lp[kinds < 7]).all() and not np.isnan(lp[kinds == 7]).any()
            worst = max(worst, check_logprobs(out["lp"][rows[slot], n[slot]], lp, bound, (name, top_k, T)))
    print(f"log-prob V={V} Vlive={Vlive} {dtype}: worst |error| / BOUND = {worst:.4f}")
    return worst


# ---- 5. the language model -----------------------------------------------------------------------------------------------------------------------
L_LM = 40
B_LM, P_LM, N_LM, PAD = DS.B_LM, DS.P_LM, DS.N_LM, DS.PAD
ACGT = [7, 8, 9, 10]
LM_MODES = ("plain", "lengths", "fanout", "lookahead")


def lm(dev):
    return DS.tiny_lm(dev, L=L_LM)


def gen(m, ids, lengths=None, N=N_LM, **kw):
    kw.setdefault("use_cache", True)
    return m.generate(ids, max_length=P_LM + N, lengths=lengths, pad_token_id=PAD, return_dict_in_generate=True, **kw)


def new_tokens(out, lengths, N=N_LM, fan=1):
    B = out.sequences.shape[0]
    start = torch.full((B,), P_LM, dtype=torch.int64) if lengths is None else lengths.cpu().long().repeat_interleave(fan)
    return out.sequences.cpu().gather(1, start[:, None] + torch.arange(N))


def mode_kwargs(mode, dev):
    ids, lengths = DS.lm_inputs(dev)
    if mode == "lengths":
        return ids, lengths, {}
    return ids, None, {"fanout": dict(num_return_sequences=2), "lookahead": dict(lookahead=4), "plain": {}}[mode]


def lm_logprob_check(out, toks, T, what):
    """logprobs against log_softmax(scores T)[token] in fp64.  scores = fl(l / T): scores T is l (1 + d), |d| <= 2^-24, and a log-softmax
    moves by at most twice the largest change of a logit, so for T != 1 the bound grows by 2 * 2^-24 max |l|; at T = 1 scores are l."""
    worst = 0.0
    V = out.scores[0].shape[1]
    for i, s in enumerate(out.scores):
        l64 = s.cpu().double().numpy() * float(np.float32(T))
        lp, bound = logprob_reference(l64, V, toks[:, i].numpy())
        if T != 1.0:
            bound = bound + 2 * E32 * np.abs(l64).max(1)
        worst = max(worst, check_logprobs(out.logprobs[:, i].cpu(), lp, bound, (what, i)))
    return worst


def case_lm_allowed_tokens(dev, mode, graphed):
    """allowed_tokens: only those ids in the new columns (on the parent commit **kwargs swallows the argument: other ids appear);
    log-probs against the scores; with ``graphed`` the replayed run against the eager one bit for bit, log-probs included"""
    m = lm(dev)
    ids, lengths, extra = mode_kwargs(mode, dev)
    fan = extra.get("num_return_sequences", 1)
    kw = dict(top_k=12, temperature=1.3, seed=5, output_scores=True, output_logprobs=True, **extra)
    free = gen(m, ids, lengths, top_k=12, temperature=1.3, seed=5, **extra)
    tf = new_tokens(free, lengths, fan=fan)
    assert bool(((tf < 7) | (tf > 10)).any())                                  # unconstrained, the model does leave A C G T
    out = gen(m, ids, lengths, allowed_tokens=ACGT, **kw)
    assert out._fields == ("sequences", "scores") + (("lengths",) if mode == "lengths" else ()) + ("logprobs",)
    toks = new_tokens(out, lengths, fan=fan)
    assert bool(((toks >= 7) & (toks <= 10)).all()), toks
    assert out.logprobs.shape == (B_LM * fan, N_LM) and out.logprobs.dtype == torch.float32
    print(f"lm {mode}: worst log-prob |error| / BOUND = {lm_logprob_check(out, toks, 1.3, mode):.4f}")
    at_one = gen(m, ids, lengths, allowed_tokens=ACGT, **dict(kw, temperature=1.0))
    print(f"lm {mode}, T = 1: worst log-prob |error| / BOUND = {lm_logprob_check(at_one, new_tokens(at_one, lengths, fan=fan), 1.0, mode):.4f}")
    if graphed:
        g = gen(m, ids, lengths, allowed_tokens=ACGT, cg=True, **kw)
        assert torch.equal(g.sequences, out.sequences) and torch.equal(torch.stack(g.scores), torch.stack(out.scores))
        assert torch.equal(g.logprobs.view(torch.int32), out.logprobs.view(torch.int32))


def case_lm_iupac(dev, graphed):
    from hyena_dna_amd.inference import iupac_constraints
    m = lm(dev)
    ids, lengths = DS.lm_inputs(dev)
    pattern = "ACGT..RY"
    c = iupac_constraints(pattern).to(dev)
    for ln in (None, lengths):
        for cg in (False, True)[:1 + graphed]:
            out = gen(m, ids, ln, N=len(pattern), constraints=c, top_k=16, temperature=2.0, seed=9, vocab_size=12, cg=cg)
            toks = new_tokens(out, ln, N=len(pattern))
            assert bool((toks[:, :4] == torch.tensor(ACGT)).all()), toks
            assert bool(((toks[:, 6] == 7) | (toks[:, 6] == 9)).all()) and bool(((toks[:, 7] == 8) | (toks[:, 7] == 10)).all()), toks
            assert bool((toks[:, 4:6] < 12).all())
    # per-row constraints, and both arguments together: the intersection
    rows = torch.stack([iupac_constraints("M" * 8), iupac_constraints("S" * 8), iupac_constraints("." * 8)]).to(dev)
    toks = new_tokens(gen(m, ids, N=8, constraints=rows, allowed_tokens=[8, 9, 10, 11], top_k=16, temperature=2.0, seed=9, sampler="device"), None, N=8)
    assert bool((toks[0] == 8).all()) and bool(((toks[1] == 8) | (toks[1] == 9)).all()) and bool(((toks[2] >= 8) & (toks[2] <= 11)).all())
    import pytest
    rows[0] = iupac_constraints("." * 5 + "M..").to(dev)
    with pytest.raises(ValueError, match="row 0, position 5"):                  # {A, C} and {G, T, N}: nothing left
        gen(m, ids, N=8, constraints=rows, allowed_tokens=[9, 10, 11])


def case_lm_min_new_tokens(dev, graphed):
    m = lm(dev)
    ids, lengths = DS.lm_inputs(dev)
    kw = dict(top_k=4, temperature=1.5, seed=21, vocab_size=12)
    free = new_tokens(gen(m, ids, **kw), None)
    eos = int(free[0, 0])                                                       # row 0 would emit it at once
    plain = new_tokens(gen(m, ids, eos_token_id=eos, **kw), None)
    assert plain[0, 0] == eos and bool((plain[0, 1:] == PAD).all())
    mnew = 6
    for cg in (False, True)[:1 + graphed]:
        out = gen(m, ids, eos_token_id=eos, min_new_tokens=mnew, cg=cg, **kw)
        got = new_tokens(out, None)
        assert bool((got[:, :mnew] != eos).all()), got
        for b in range(B_LM):                                                   # from position m on eos is allowed again and ends the row
            hit = (got[b, mnew:] == eos).nonzero()
            if len(hit):
                assert bool((got[b, mnew + int(hit[0]) + 1:] == PAD).all())
    import pytest
    with pytest.raises(ValueError, match="eos_token_id"):
        gen(m, ids, min_new_tokens=3, seed=1)


def case_lm_all_ones_is_todays_generate(dev, ragged):
    m = lm(dev)
    ids, lengths = DS.lm_inputs(dev)
    lengths = lengths if ragged else None
    kw = dict(top_k=4, top_p=0.9, temperature=1.3, seed=11, output_scores=True)
    ref = gen(m, ids, lengths, **kw)
    ones = torch.full((N_LM,), -1, dtype=torch.int64).to(dev)
    for c in (ones, ones[None].repeat(B_LM, 1)):
        out = gen(m, ids, lengths, constraints=c, **kw)
        assert out._fields == ref._fields
        assert torch.equal(out.sequences, ref.sequences) and torch.equal(torch.stack(out.scores), torch.stack(ref.scores))
    out = gen(m, ids, lengths, allowed_tokens=range(16), output_logprobs=True, **kw)
    assert torch.equal(out.sequences, ref.sequences) and torch.equal(torch.stack(out.scores), torch.stack(ref.scores))


def case_lm_stop_check(dev):
    """stop_check_every with log-probs: (B, number of steps run), NaN for the positions of a finished row"""
    m = lm(dev)
    ids, _ = DS.lm_inputs(dev)
    kw = dict(top_k=4, temperature=1.5, seed=21, vocab_size=12, allowed_tokens=ACGT, output_logprobs=True)
    toks = new_tokens(gen(m, ids, **kw), None)
    cands = [t for t in ACGT if all((toks[b] == t).any() for b in range(B_LM))]
    assert cands, toks
    eos = min(cands, key=lambda t: max(int((toks[b] == t).nonzero()[0]) for b in range(B_LM)))
    first = [int((toks[b] == eos).nonzero()[0]) for b in range(B_LM)]
    full = gen(m, ids, eos_token_id=eos, **kw)
    early = gen(m, ids, eos_token_id=eos, stop_check_every=1, **kw)
    assert early.logprobs.shape == (B_LM, max(first) + 1) and full.logprobs.shape == (B_LM, N_LM)
    assert torch.equal(early.sequences, full.sequences)
    for b in range(B_LM):
        assert not torch.isnan(full.logprobs[b, :first[b] + 1]).any() and torch.isnan(full.logprobs[b, first[b] + 1:]).all()
        assert torch.equal(early.logprobs[b, :first[b] + 1], full.logprobs[b, :first[b] + 1])


def case_lm_refusals(dev):
    import pytest
    m = lm(dev)
    ids, lengths = DS.lm_inputs(dev)
    N = 4
    ok = torch.full((N,), -1, dtype=torch.int64).to(dev)
    for kw in (dict(allowed_tokens=ACGT), dict(constraints=ok), dict(min_new_tokens=2), dict(output_logprobs=True)):
        with pytest.raises(ValueError, match="sampler='device'"):
            gen(m, ids, N=N, sampler="torch", **kw)
    with pytest.raises(ValueError, match="use_cache=True"):                    # each of them selects the device sampler
        m.generate(ids, max_length=P_LM + N, allowed_tokens=ACGT)
    empty = ok.clone()
    empty[2] = 0xF000                                                           # bits 12 .. 15 only: nothing below vocab_size = 12
    with pytest.raises(ValueError, match="position 2"):
        gen(m, ids, N=N, constraints=empty, vocab_size=12)
    per_row = ok[None].repeat(B_LM, 1).clone()
    per_row[1, 3] = 0
    with pytest.raises(ValueError, match="row 1, position 3"):
        gen(m, ids, N=N, constraints=per_row)
    for bad in (ok[:3], ok[None].repeat(2, 1), ok[None, None]):
        with pytest.raises(ValueError, match="constraints must be"):
            gen(m, ids, N=N, constraints=bad)
    for bad in (ok.int(), ok.float(), ok.tolist()):
        with pytest.raises(ValueError, match="int64"):
            gen(m, ids, N=N, constraints=bad)
    for bad in ([7, 16], [-1]):
        with pytest.raises(ValueError, match="allowed_tokens"):
            gen(m, ids, N=N, allowed_tokens=bad)
    with pytest.raises(ValueError, match="allow no token"):
        gen(m, ids, N=N, allowed_tokens=[12, 13], vocab_size=12)
    with pytest.raises(ValueError, match="min_new_tokens"):
        gen(m, ids, N=N, min_new_tokens=-1, eos_token_id=1)


# ---- 6. the C entry point's refusals -------------------------------------------------------------------------------------------------------------
def case_abi_refusals(_lib, dev):
    import ctypes
    L = _lib.lib()
    B, V, ncols = 2, 16, 8
    t = dict(logits=torch.zeros(B, V), seed=torch.zeros(1, dtype=torch.int64), col=torch.zeros(B, dtype=torch.int32),
             done=torch.zeros(B, dtype=torch.int32), seq=torch.zeros(B, ncols, dtype=torch.int64), nxt=torch.zeros(B, dtype=torch.int64),
             allow=torch.full((B, ncols), -1, dtype=torch.int64), start=torch.zeros(B, dtype=torch.int32), lp=torch.zeros(B, ncols))
    t = {k: v.to(dev) for k, v in t.items()}

    def call(**kw):
        a = dict(logits=t["logits"].data_ptr(), ldl=V, dtype=0, B=B, V=V, Vlive=12, T=1.0, top_k=4, top_p=0.9, seed=t["seed"].data_ptr(), eos=-1,
                 pad=0, col=t["col"].data_ptr(), done=t["done"].data_ptr(), seq=t["seq"].data_ptr(), lds=ncols, ncols=ncols, nxt=t["nxt"].data_ptr(),
                 ldn=1, allow=t["allow"].data_ptr(), lda=ncols, nallow=ncols, start=t["start"].data_ptr(), lp=t["lp"].data_ptr(), ldp=ncols)
        a.update(kw)
        return L.hyena_decode_sample_constrained(a["logits"], a["ldl"], a["dtype"], a["B"], a["V"], a["Vlive"], ctypes.c_float(a["T"]),
                                                 a["top_k"], ctypes.c_float(a["top_p"]), a["seed"], a["eos"], a["pad"], a["col"], a["done"],
                                                 a["seq"], a["lds"], a["ncols"], a["nxt"], a["ldn"], None, None, a["allow"], a["lda"],
                                                 a["nallow"], a["start"], a["lp"], a["ldp"], None)

    for name in ("logits", "seed", "col", "done", "seq", "nxt", "start"):
        assert call(**{name: None}) == 1, name
    for kw in (dict(V=65, ldl=65), dict(Vlive=0), dict(Vlive=17), dict(top_p=0.0), dict(top_p=1.5), dict(dtype=3), dict(ldl=V - 1),
               dict(lds=ncols - 1), dict(nallow=0), dict(lda=ncols - 1), dict(lda=-1), dict(ldp=0), dict(start=None, allow=None),
               dict(start=None, lp=None)):
        assert call(**kw) == 1, kw
    assert (t["seq"] == 0).all() and (t["col"] == 0).all() and (t["lp"] == 0).all()      # nothing ran
    if dev == "cpu":                                                            # (the emulation: the good calls really run)
        assert call() == 0 and t["col"].tolist() == [1, 1]
        assert call(start=None, allow=None, lp=None) == 0 and call(lda=0) == 0 and t["col"].tolist() == [3, 3]
