"""Beam search for cached generation -- csrc/decode_kernels.h decode_beam_kernel / decode_reorder_fan_kernel / decode_beam_backtrack_kernel,
include/hyena_decode.h hyena_decode_beam / _reorder_fan / _beam_backtrack, HyenaDecodeState.reorder, inference.BeamSearcher,
generate(num_beams=k) -- held to torch / fp64 restatements of its specification.  The cases live here and run twice: under tests/hipemu on
the CPU (test_decode_beam_emu.py) and on the gfx950 binary (test_gpu_decode_beam.py).

Reorder.  Bit for bit against index_select on clones; the whole tensors are compared, so every element outside [c0, *pos) -- the columns
below c0, from *pos on and the pad of the pitch, all filled with random values -- must come back unchanged.

Beam step.  The kernel's log-prob is decode_sample_con_kernel's, so decode_constrain_local.logprob_reference gives lp* and its BOUND; a
candidate's score is fl(score + lp): TAU = BOUND + 1.01 * 2^-24 |score + lp*| + 2^-100 (one fp32 rounding of the sum).
  (a) every written score lies within TAU of its parent's score plus the fp64 log-prob of its token;
  (b) the selection is optimal up to TAU: no candidate left out beats the worst selected one by more than the sum of their TAUs, the ranks
      descend within the TAUs of neighbours; where the reference's k-th and (k + 1)-th scores are further apart than their TAUs the
      selected SET is the reference's (otherwise the group is "undecided": counted, at most 1 % of the groups);
  (c) -inf scores and NaN scores are compared exactly: all numbers before every NaN, -inf after every finite number, and within the -inf
      and the NaN candidates the lowest flat indices j V + i, in order;  parent / done / next / col and the three records follow the
      header's rules exactly;  a finished row has one candidate, `pad`, with its score unchanged bit for bit;
  (d) rows of NaN, +inf and all -inf logits: NaN log-probs, so NaN scores, which rank last; k candidates are still chosen and every
      token is < Vlive or pad (the same checker: it never assumes a finite value).

LM.  A beam's score against the teacher-forced sum of log-softmax (fp64, from the fp32 logits of ONE full forward over the beam's own
sequence, live columns only).  Tolerance per step: TAU of the step plus 2 * TOL * max |l|, TOL = 1e-5 the fp32 logit tolerance of
tests/test_gpu_decode_fan.py for cached against full logits (under autocast its 2e-2) -- a log-softmax moves by at most twice the largest
change of a logit."""
import numpy as np
import torch

from tests import decode_constrain_local as DC
from tests import decode_sample_local as DS

DTYPES = DS.DTYPES
E32 = DC.E32
CHUNK = 8192
NCOLS = 12                                                                       # the beam cases' sequence has columns [0, NCOLS)
VSHAPES = [(16, 12), (16, 16), (64, 64)]
KS = (1, 2, 3, 8, 16)
GS = (1, 3)
ACGT = DC.ACGT
PAD = DS.PAD


# ---- 1. the reorder kernel --------------------------------------------------------------------------------------------------------------------
REORDER_SHAPES = [(2, 3, 5, 8192 + 40, 8192, 8195, 8204), (1, 16, 64, 48, 0, 5, 48), (3, 2, 3, 24, 0, 1, 2)]       # (G, fan, D, Lcap, S, c0, *pos)
REORDER_SHAPE_WIDE = (2, 8, 256, 8192 + 320, 8192, 8200, 8500)                                                      # several workgroups
PARENT_KINDS = ("identity", "cyclic", "one", "random", "outside")


def make_parents(kind, G, fan, seed=0):
    g = torch.Generator().manual_seed(seed)
    base = (torch.arange(G) * fan)[:, None]
    j = torch.arange(fan)[None].repeat(G, 1)
    if kind == "cyclic":                                                         # every row is overwritten by a row that is itself overwritten
        j = (j + 1) % fan
    elif kind == "one":
        j = torch.full_like(j, fan // 2)
    elif kind in ("random", "outside"):
        j = torch.randint(0, fan, (G, fan), generator=g)
    p = (base + j).reshape(-1).to(torch.int32)
    effective = p.clone()
    if kind == "outside":                                                        # one parent outside its group: that row stays as it is
        b = (G * fan) // 2
        p[b] = G * fan + 3 if G == 1 else ((b // fan + 1) % G) * fan
        effective[b] = b
        p[0], effective[0] = -1, 0
    return p, effective


class ReorderCase:
    def __init__(self, _lib, dev, shape, dtype, seed=0):
        G, fan, D, Lcap, S, c0, pos = shape
        self.shape, self.B = shape, G * fan
        g = torch.Generator().manual_seed(seed)
        ldr = _lib.row_pitch(max(Lcap - S, 1))
        self.hist = torch.randn(self.B, D, ldr, generator=g).to(dtype).to(dev)              # every element a canary: columns, the rest, the pad
        self.shared = torch.randn(G, D, _lib.row_pitch(S), generator=g).to(dtype).to(dev) if S else None
        self.tail = torch.randn(3 * D, self.B, 2, generator=g).to(dev)
        self.pos = torch.tensor([pos], dtype=torch.int32).to(dev)

    def run(self, _lib, parents):
        G, fan, D, Lcap, S, c0, pos = self.shape
        _lib.decode_reorder_fan(self.hist, self.tail, parents.to(self.hist.device), self.pos, self.B, fan, Lcap, S, c0)


def case_reorder(_lib, dev, shape, dtype, kinds=PARENT_KINDS):
    G, fan, D, Lcap, S, c0, pos = shape
    for n, kind in enumerate(kinds):
        c = ReorderCase(_lib, dev, shape, dtype, seed=n)
        parents, eff = make_parents(kind, G, fan, seed=n)
        want_h, want_t = c.hist.clone(), c.tail.clone()
        idx = eff.long().to(dev)
        want_h[:, :, c0 - S:pos - S] = c.hist.index_select(0, idx)[:, :, c0 - S:pos - S]
        want_t.copy_(c.tail.index_select(1, idx))
        shared = None if c.shared is None else c.shared.clone()
        c.run(_lib, parents)
        assert torch.equal(c.hist.view(torch.int16 if dtype != torch.float32 else torch.int32),
                           want_h.view(torch.int16 if dtype != torch.float32 else torch.int32)), kind
        assert torch.equal(c.tail, want_t), kind
        assert c.pos.item() == pos and (shared is None or torch.equal(shared, c.shared))
        if kind == "cyclic" and fan > 1:
            assert not torch.equal(want_h, ReorderCase(_lib, dev, shape, dtype, seed=n).hist)     # (the case does move something)


def case_reorder_parked(_lib, dev, dtype):
    """*pos outside [S, Lcap]: nothing at all changes, the tail included"""
    shape = REORDER_SHAPES[0]
    G, fan, D, Lcap, S, c0, _ = shape
    for pos in (-1, S - 1, Lcap + 1):
        c = ReorderCase(_lib, dev, shape[:6] + (pos,), dtype, seed=pos % 7)
        h, t = c.hist.clone(), c.tail.clone()
        c.run(_lib, make_parents("cyclic", G, fan)[0])
        assert torch.equal(c.hist, h) and torch.equal(c.tail, t) and c.pos.item() == pos, pos


def case_reorder_refusals(_lib, dev):
    L = _lib.lib()
    G, fan, D, Lcap, S, c0 = 2, 2, 2, 8300, 8192, 8200
    B = G * fan
    hr = torch.zeros(B, D, _lib.row_pitch(Lcap - S)).to(dev)
    tail, parent = torch.ones(3 * D, B, 2).to(dev), torch.tensor([1, 0, 3, 2], dtype=torch.int32).to(dev)
    pos = torch.tensor([-1], dtype=torch.int32).to(dev)                         # a parked position: a good call does nothing
    p = lambda t: t.data_ptr()

    def call(hr_ptr=p(hr), tail_ptr=p(tail), parent_ptr=p(parent), pos_ptr=p(pos), B=B, Bcap=B, fan=fan, D=D, Lcap=Lcap, S=S, c0=c0,
             ldr=hr.stride(1), dtype=0):
        return L.hyena_decode_reorder_fan(hr_ptr, tail_ptr, parent_ptr, pos_ptr, B, Bcap, fan, D, Lcap, S, c0, ldr, dtype, None)

    assert call() == 0
    for kw in (dict(hr_ptr=None), dict(tail_ptr=None), dict(parent_ptr=None), dict(pos_ptr=None), dict(hr_ptr=p(hr) + 4), dict(B=3), dict(B=0),
               dict(fan=0), dict(fan=17, B=34, Bcap=34), dict(Bcap=B - 1), dict(S=100), dict(S=16384), dict(c0=S - 1), dict(c0=Lcap + 1),
               dict(ldr=hr.stride(1) + 4), dict(ldr=8), dict(dtype=3), dict(D=0), dict(Lcap=(1 << 20) + 1)):
        assert call(**kw) == 1, kw
    assert bool((tail == 1).all()) and pos.item() == -1


# ---- 2. the beam kernel -----------------------------------------------------------------------------------------------------------------------
def run_beam(_lib, dev, logits, score, done, col, start, k, Vlive, eos=-1, pad=0, allow=None, nrec=6):
    """one call on copies of the state and sentinel-filled outputs -> dict of CPU tensors"""
    B = logits.shape[0]
    o = dict(score=score.clone().to(dev), done=done.clone().to(dev), col=col.clone().to(dev),
             parent=torch.full((B,), -5, dtype=torch.int32).to(dev), nxt=torch.full((B, 1), -9, dtype=torch.int64).to(dev),
             tok_hist=torch.full((B, nrec), -3, dtype=torch.int32).to(dev), parent_hist=torch.full((B, nrec), -4, dtype=torch.int32).to(dev),
             lp_hist=torch.full((B, nrec), -777.0).to(dev))
    _lib.decode_beam(logits.to(dev), o["score"], o["col"], o["done"], start.to(dev), o["parent"], o["nxt"], k, NCOLS, eos=eos, pad=pad,
                     vocab=Vlive, allow=None if allow is None else allow.to(dev), tok_hist=o["tok_hist"], parent_hist=o["parent_hist"],
                     lp_hist=o["lp_hist"])
    o = {n: t.cpu() for n, t in o.items()}
    o["nxt"] = o["nxt"][:, 0]
    return o


def lp_matrix(l64, Vlive):
    """(B, V) float64 logits -> lp* (B, Vlive), BOUND (B, Vlive): decode_constrain_local.logprob_reference for every token"""
    B = len(l64)
    lp, bd = np.full((B, Vlive), np.nan), np.zeros((B, Vlive))
    for i in range(Vlive):
        lp[:, i], bd[:, i] = DC.logprob_reference(l64, Vlive, np.full(B, i))
    return lp, bd


def _klass(s):
    return 2 if np.isnan(s) else (0 if np.isfinite(s) else 1)


def check_beam(o, logits, score, done, col, start, A, k, Vlive, eos, pad, nrec, stats):
    """every rule of the header against the fp64 restatement; ``A`` bool (B, V) the allowed sets; ``stats``: dict(groups, undecided)"""
    l64 = logits.double().numpy()
    B, V = l64.shape
    lp, bd = lp_matrix(l64, Vlive)
    sc, dn, cl, st = score.double().numpy(), done.numpy(), col.numpy(), start.numpy()
    for g in range(B // k):
        b0, c = g * k, int(cl[g * k])
        rows = slice(b0, b0 + k)
        if c < 0 or c >= NCOLS:                                                  # parked: untouched
            assert torch.equal(o["score"][rows].view(torch.int32), score[rows].view(torch.int32)) and torch.equal(o["done"][rows], done[rows])
            assert torch.equal(o["col"][rows], col[rows]) and bool((o["parent"][rows] == -5).all()) and bool((o["nxt"][rows] == -9).all())
            assert bool((o["tok_hist"][rows] == -3).all()) and bool((o["parent_hist"][rows] == -4).all()) and bool((o["lp_hist"][rows] == -777.0).all())
            continue
        cand = {}                                                                # flat index -> (score*, TAU, row, token, lp*, BOUND, finished)
        with np.errstate(invalid="ignore"):
            for j in range(k):
                b = b0 + j
                if dn[b]:
                    cand[j * V] = (sc[b], 0.0, j, pad, 0.0, 0.0, True)
                    continue
                for i in range(Vlive):
                    if A[b, i]:
                        s = sc[b] + lp[b, i]
                        tau = bd[b, i] + 1.01 * E32 * abs(s) + 2.0 ** -100 if np.isfinite(s) else 0.0
                        cand[j * V + i] = (s, tau, j, i, lp[b, i], bd[b, i], False)
        assert len(cand) >= k
        picked = []
        for r in range(k):
            b = b0 + r
            pj, tok = int(o["parent"][b]) - b0, int(o["nxt"][b])
            assert 0 <= pj < k, (g, r, pj)
            fin = bool(dn[b0 + pj])
            flat = pj * V if fin else pj * V + tok
            assert (tok == pad) if fin else (0 <= tok < Vlive), (g, r, tok)
            assert flat in cand and flat not in picked, (g, r, flat)            # an allowed token of a live row, or the pad of a finished one; once
            s, tau, _, _, lps, lpb, _ = cand[flat]
            got = float(o["score"][b])
            # (a) the written score; (c) exactly where it must be
            if fin:
                assert torch.equal(o["score"][b].view(torch.int32), score[b0 + pj].view(torch.int32))
            elif np.isfinite(s):
                assert abs(got - s) <= tau, (g, r, got, s, tau)
            else:
                assert (np.isnan(got) and np.isnan(s)) or got == s, (g, r, got, s)
            assert int(o["done"][b]) == (1 if fin or tok == eos else 0) and int(o["col"][b]) == c + 1
            n = c - int(st[b])
            if 0 <= n < nrec:
                assert int(o["tok_hist"][b, n]) == tok and int(o["parent_hist"][b, n]) == b0 + pj
                glp = float(o["lp_hist"][b, n])
                if fin:
                    assert glp == 0.0
                elif np.isfinite(lps):
                    assert abs(glp - lps) <= lpb, (g, r, glp, lps)
                else:
                    assert (np.isnan(glp) and np.isnan(lps)) or glp == lps
                wrote = 1
            else:
                wrote = 0
            for name, sentinel in (("tok_hist", -3), ("parent_hist", -4), ("lp_hist", -777.0)):
                assert int((o[name][b] != sentinel).sum()) == wrote, (name, g, r)
            picked.append(flat)
        # (b), (c): the selection
        ks = [_klass(cand[f][0]) for f in picked]
        assert ks == sorted(ks), (g, ks)                                         # finite numbers, then -inf, then NaN
        for kl in (0, 1, 2):
            pool = sorted(f for f in cand if _klass(cand[f][0]) == kl)
            mine = [f for f in picked if _klass(cand[f][0]) == kl]
            if any(x > kl for x in ks):
                assert len(mine) == len(pool), (g, kl)                           # a later class only once this one is used up
            if kl > 0:
                assert mine == pool[:len(mine)], (g, kl, mine, pool[:len(mine)])  # bit-equal scores rank by flat index
                continue
            if not mine:
                continue
            for x, y in zip(mine, mine[1:]):                                     # descending within the bounds
                assert cand[x][0] >= cand[y][0] - (cand[x][1] + cand[y][1]), (g, x, y)
                if cand[x][0] == cand[y][0] and cand[x][1] == 0.0 and cand[y][1] == 0.0:
                    assert x < y
            worst = min(mine, key=lambda f: cand[f][0])
            for f in pool:
                if f not in mine:
                    assert cand[f][0] <= cand[worst][0] + cand[f][1] + cand[worst][1], (g, f, worst)
            stats["groups"] += 1
            if len(pool) > len(mine):
                order = sorted(pool, key=lambda f: (-cand[f][0], f))
                x, y = order[len(mine) - 1], order[len(mine)]
                # a pair (selected u, left out v) is open when the bounds cannot tell them apart -- unless they are one row's candidates of
                # equal logits (16-bit logits repeat values): those scores are bit-equal in the kernel too and the flat index decides
                near_in = [u for u in order[:len(mine)] if cand[u][0] <= cand[x][0] + 1e-3]
                near_out = [v for v in order[len(mine):] if cand[v][0] >= cand[y][0] - 1e-3]
                if any(cand[u][0] - cand[v][0] <= cand[u][1] + cand[v][1] and not (cand[u][2] == cand[v][2] and cand[u][0] == cand[v][0])
                       for u in near_in for v in near_out):
                    stats["undecided"] += 1
                else:
                    assert set(mine) == set(order[:len(mine)]), (g, mine, order[:len(mine)])


def beam_inputs(V, Vlive, k, G, dtype, state, seed):
    g = torch.Generator().manual_seed(seed)
    B = G * k
    logits = (torch.randn(B, V, generator=g) * 2.0).to(dtype)
    if state == "first":
        score = torch.full((G, k), float("-inf"))
        score[:, 0] = 0.0
        score = score.reshape(B)
    else:
        score = torch.randn(B, generator=g) * 2.0 - 6.0
    return logits, score, g


def all_live(B, V, Vlive):
    return np.tile(np.arange(V) < Vlive, (B, 1))


def case_beam(_lib, dev, V, Vlive, dtype):
    """k x G x state x flavour against the restatement; prints and bounds the number of undecided groups"""
    stats = dict(groups=0, undecided=0)
    seed = 1000 * V + 10 * Vlive
    for k in KS:
        for G in GS:
            for state in ("first", "random"):
                seed += 1
                B = G * k
                logits, score, g = beam_inputs(V, Vlive, k, G, dtype, state, seed)
                zeros = torch.zeros(B, dtype=torch.int32)
                col = torch.full((B,), 4, dtype=torch.int32)
                # plain
                o = run_beam(_lib, dev, logits, score, zeros, col, zeros, k, Vlive)
                check_beam(o, logits, score, zeros, col, zeros, all_live(B, V, Vlive), k, Vlive, -1, 0, 6, stats)
                # finished rows, eos, a parked group, records shorter than n for half of the rows
                done = (torch.rand(B, generator=g) < 0.3).int()
                colp = col.clone()
                if G > 1:
                    colp[k:2 * k] = (-1, NCOLS)[k % 2]
                start = torch.where(torch.arange(B) % 2 == 0, 0, 3).int()         # n = 4 (outside the record of 3) or 1
                eos = int(logits[0, :Vlive].float().argmax())
                o = run_beam(_lib, dev, logits, score, done, colp, start, k, Vlive, eos=eos, pad=1, nrec=3)
                check_beam(o, logits, score, done, colp, start, all_live(B, V, Vlive), k, Vlive, eos, 1, 3, stats)
                # masks per row (random; every fourth empty, every fourth + 1 with dead bits only) and one row of masks for the batch
                m = np.random.default_rng(seed).integers(0, 2 ** 64, size=(B, 5), dtype=np.uint64)
                m[0::4] = 0
                if Vlive < 64:
                    m[1::4] = np.uint64(1) << np.uint64(63)
                startm = torch.from_numpy(np.random.default_rng(seed + 1).integers(0, 7, size=B).astype(np.int32))       # n = 4 - start: -2 ... 4
                for allow in (m, m[0] | np.uint64(1 << 2)):
                    A = DC.allowed_sets(allow, startm.numpy(), col.numpy(), Vlive, V)
                    o = run_beam(_lib, dev, logits, score, done, col, startm, k, Vlive, eos=eos, pad=1, allow=DC.masks_to_tensor(allow))
                    check_beam(o, logits, score, done, col, startm, A, k, Vlive, eos, 1, 6, stats)
    print(f"beam V={V} Vlive={Vlive} {dtype}: {stats['undecided']} of {stats['groups']} groups undecided")
    assert stats["undecided"] * 100 <= stats["groups"]
    return stats


def case_beam_ties(_lib, dev, dtype):
    """equal logits and equal scores give bit-equal candidates: they rank by the flat index j V + i"""
    V, Vlive, k, G = 16, 12, 3, 2
    B = G * k
    logits = torch.full((B, V), 0.75).to(dtype)
    score = torch.full((B,), -2.5)
    zeros, col = torch.zeros(B, dtype=torch.int32), torch.full((B,), 2, dtype=torch.int32)
    o = run_beam(_lib, dev, logits, score, zeros, col, zeros, k, Vlive)
    assert o["parent"].tolist() == [0, 0, 0, 3, 3, 3] and o["nxt"].tolist() == [0, 1, 2, 0, 1, 2]
    assert len(set(o["score"].tolist())) == 1
    allow = torch.full((4,), (1 << 5) | (1 << 9), dtype=torch.int64)             # two tokens per row: row 0's two, then row 1's first
    o = run_beam(_lib, dev, logits, score, zeros, col, zeros, k, Vlive, allow=allow)
    assert o["parent"].tolist() == [0, 0, 1, 3, 3, 4] and o["nxt"].tolist() == [5, 9, 5, 5, 9, 5]
    done = torch.tensor([1, 0, 0, 0, 1, 0], dtype=torch.int32)                   # a finished row: ONE candidate, pad; its score above the others'
    hi = score.clone()
    hi[0] = hi[4] = 0.0
    o = run_beam(_lib, dev, logits, hi, done, col, zeros, k, Vlive, pad=7)
    assert o["parent"].tolist() == [0, 1, 1, 4, 3, 3] and o["nxt"].tolist() == [7, 0, 1, 7, 0, 1] and o["done"].tolist() == [1, 0, 0, 1, 0, 0]
    assert o["score"][0] == 0.0 and o["score"][3] == 0.0 and o["lp_hist"][0, 2] == 0.0
    stats = dict(groups=0, undecided=0)
    check_beam(o, logits, hi, done, col, zeros, all_live(B, V, Vlive), k, Vlive, -1, 7, 6, stats)


def case_beam_nonfinite(_lib, dev, V, Vlive, dtype):
    """(d): NaN, +inf and all -inf rows among clean ones, and groups without a single clean row"""
    stats = dict(groups=0, undecided=0)
    nan, inf = float("nan"), float("inf")
    for k in (1, 2, 3, 8, 16):
        G = 4
        B = G * k
        logits, score, g = beam_inputs(V, Vlive, k, G, dtype, "random", 77 + k)
        for b in range(B):
            kind = b % 6 if b >= k else 1 + b % 3                                # group 0: no clean row at all
            if kind == 1:
                logits[b, (b + 1) % Vlive] = nan
            elif kind == 2:
                logits[b, (b + 2) % Vlive] = inf
            elif kind == 3:
                logits[b, :Vlive] = -inf
            elif kind == 4:
                logits[b, b % Vlive] = -inf                                       # one token of probability 0: a -inf candidate among numbers
        zeros, col = torch.zeros(B, dtype=torch.int32), torch.full((B,), 1, dtype=torch.int32)
        for state_score in (score, torch.where(torch.arange(B) % k == 0, 0.0, -inf)):
            o = run_beam(_lib, dev, logits, state_score, zeros, col, zeros, k, Vlive, eos=2, pad=1)
            assert bool(((o["nxt"] >= 0) & (o["nxt"] < Vlive)).all()) and bool((o["col"] == 2).all())
            assert bool(torch.isnan(o["score"][:k]).all())                        # group 0: every candidate is NaN, k are chosen all the same
            assert o["parent"][:k].tolist() == [0] * min(k, Vlive) + [1] * (k - min(k, Vlive)) or k > 2 * Vlive
            check_beam(o, logits, state_score, zeros, col, zeros, all_live(B, V, Vlive), k, Vlive, 2, 1, 6, stats)
    return stats


def case_beam_refusals(_lib, dev):
    L = _lib.lib()
    B, fan, V, nrec = 4, 2, 16, 6
    t = dict(logits=torch.zeros(B, V), col=torch.zeros(B, dtype=torch.int32), done=torch.zeros(B, dtype=torch.int32), score=torch.zeros(B),
             start=torch.zeros(B, dtype=torch.int32), parent=torch.full((B,), -5, dtype=torch.int32), nxt=torch.zeros(B, dtype=torch.int64),
             allow=torch.full((B, nrec), -1, dtype=torch.int64), th=torch.zeros(B, nrec, dtype=torch.int32),
             ph=torch.zeros(B, nrec, dtype=torch.int32), lh=torch.zeros(B, nrec))
    t = {n: v.to(dev) for n, v in t.items()}

    def call(**kw):
        a = dict(logits=t["logits"].data_ptr(), ldl=V, dtype=0, B=B, fan=fan, V=V, Vlive=12, eos=-1, pad=0, col=t["col"].data_ptr(),
                 done=t["done"].data_ptr(), score=t["score"].data_ptr(), start=t["start"].data_ptr(), parent=t["parent"].data_ptr(),
                 nxt=t["nxt"].data_ptr(), ldn=1, ncols=8, allow=t["allow"].data_ptr(), lda=nrec, nallow=nrec, th=t["th"].data_ptr(),
                 ph=t["ph"].data_ptr(), lh=t["lh"].data_ptr(), ldh=nrec, nrec=nrec)
        a.update(kw)
        return L.hyena_decode_beam(a["logits"], a["ldl"], a["dtype"], a["B"], a["fan"], a["V"], a["Vlive"], a["eos"], a["pad"], a["col"], a["done"],
                                   a["score"], a["start"], a["parent"], a["nxt"], a["ldn"], a["ncols"], a["allow"], a["lda"], a["nallow"], a["th"],
                                   a["ph"], a["lh"], a["ldh"], a["nrec"], None)

    for name in ("logits", "col", "done", "score", "start", "parent", "nxt"):
        assert call(**{name: None}) == 1, name
    for kw in (dict(fan=0), dict(fan=17, B=34), dict(B=3), dict(B=0), dict(V=65, ldl=65), dict(Vlive=0), dict(Vlive=17), dict(dtype=3),
               dict(ldl=V - 1), dict(ncols=0), dict(ldn=0), dict(nallow=0), dict(lda=nrec - 1), dict(lda=-1), dict(nrec=0), dict(ldh=nrec - 1)):
        assert call(**kw) == 1, kw
    assert bool((t["col"] == 0).all()) and bool((t["parent"] == -5).all())      # nothing ran
    seq = torch.zeros(B, 8, dtype=torch.int64).to(dev)
    lp = torch.zeros(B, nrec).to(dev)

    def back(**kw):
        a = dict(th=t["th"].data_ptr(), ph=t["ph"].data_ptr(), lh=t["lh"].data_ptr(), ldh=nrec, B=B, fan=fan, n_done=nrec, n_ret=2,
                 seq=seq.data_ptr(), lds=8, P=2, lp=lp.data_ptr(), ldp=nrec)
        a.update(kw)
        return L.hyena_decode_beam_backtrack(a["th"], a["ph"], a["lh"], a["ldh"], a["B"], a["fan"], a["n_done"], a["n_ret"], a["seq"], a["lds"],
                                             a["P"], a["lp"], a["ldp"], None)

    for kw in (dict(th=None), dict(ph=None), dict(seq=None), dict(lh=None), dict(fan=0), dict(B=3), dict(n_ret=0), dict(n_ret=3), dict(n_done=-1),
               dict(n_done=nrec + 1), dict(P=3), dict(P=-1), dict(ldp=nrec - 1)):
        assert back(**kw) == 1, kw
    if dev == "cpu":                                                             # (the emulation: the good calls really run)
        assert call() == 0 and t["col"].tolist() == [1] * B and call(allow=None, th=None, ph=None, lh=None) == 0
        assert back(n_done=1) == 0 and back(lp=None, lh=None, n_done=1) == 0


def case_backtrack(_lib, dev):
    """the records of a hand-made search of G = 2, k = 3, four steps -> the sequences of the final rows; parents out of range: the row itself"""
    G, k, N, P = 2, 3, 4, 2
    B = G * k
    g = torch.Generator().manual_seed(3)
    tok = torch.randint(0, 12, (B, N + 2), generator=g, dtype=torch.int32)
    par = (torch.randint(0, k, (B, N + 2), generator=g) + (torch.arange(B) // k * k)[:, None]).to(torch.int32)
    par[1, 2], par[4, 1] = -1, B                                                 # clamped: the row itself
    lp = torch.randn(B, N + 2, generator=g)
    for n_ret in (1, 2, 3):
        seq = torch.full((G * n_ret, P + N + 1), -7, dtype=torch.int64).to(dev)
        out = torch.full((G * n_ret, N), -777.0).to(dev)
        _lib.decode_beam_backtrack(tok.to(dev), par.to(dev), lp.to(dev), k, N, n_ret, seq, P, logprobs=out)
        for q in range(G * n_ret):
            b = q // n_ret * k + q % n_ret
            want_t, want_l = [0] * N, [0.0] * N
            for i in range(N - 1, -1, -1):
                want_t[i], want_l[i] = int(tok[b, i]), float(lp[b, i])
                p = int(par[b, i])
                b = p if 0 <= p < B else b
            assert seq[q].cpu().tolist() == [-7] * P + want_t + [-7] and out[q].cpu().tolist() == want_l, (n_ret, q)


# ---- 3. the operator: reorder inside a live cache ------------------------------------------------------------------------------------------------
def _layer(l_max):
    return dict(l_max=l_max, order=2, filter_order=64, emb_dim=5, short_filter_order=3, modulate=True, w=10, lr=6e-4, wd=0.0, lr_pos_emb=0.0)


def case_operator_reorder(dev, P, dtype=torch.float32, steps=10):
    """a fan cache (k = 3, G = 2): `steps` steps of random x2 per row with a random in-group reorder after each; then every final row's
    lineage of inputs replayed through a plain cache that starts from the same prefill: z of the last step and the row's history columns
    [P, t) equal bit for bit"""
    from hyena_dna_amd.hyena import HyenaOperator
    from hyena_dna_amd.inference import InferenceParams
    G, k, D = 2, 3, 8
    B, L = G * k, P + steps
    torch.manual_seed(P)
    op = HyenaOperator(d_model=D, **_layer(L + 2)).to(dev).to(dtype).eval()
    g = torch.Generator().manual_seed(P + 1)
    with torch.no_grad():
        fan = op.allocate_inference_cache(B, L, dtype=dtype, fan=k, prompt_len=P)
        ip = InferenceParams(max_seqlen=L, max_batch_size=B)
        ip.key_value_memory_dict[op._decode_key()] = fan
        op(torch.randn(G, P, D, generator=g).to(dtype).to(dev), inference_params=ip)
        S = fan.S
        assert S == P // CHUNK * CHUNK and fan.pos.item() == P
        plain = op.allocate_inference_cache(B, L, dtype=dtype)
        if S:
            plain.hist[:, :, :S].copy_(fan.hist_shared[:, :, :S].repeat_interleave(k, 0))
        plain.hist[:, :, S:P].copy_(fan.hist[:, :, :P - S])
        plain.tail.copy_(fan.tail)
        plain.pos.fill_(P)
        shared = None if fan.hist_shared is None else fan.hist_shared.clone()
        below = fan.hist[:, :, :P - S].clone()
        lineage = [[] for _ in range(B)]
        z_of = None
        for i in range(steps):
            x2 = torch.randn(B, 3 * D, generator=g).to(dtype).to(dev)
            z = fan.step(x2).clone()
            parents = (torch.randint(0, k, (B,), generator=g) + torch.arange(B) // k * k).to(torch.int32)
            fan.reorder(parents.to(dev))
            lineage = [lineage[p] + [x2[p]] for p in parents.tolist()]
            z_of = z[parents.long().to(dev)]
        assert fan.pos.item() == L
        for i in range(steps):
            zp = plain.step(torch.stack([lineage[b][i] for b in range(B)]))
        view = torch.int32 if dtype == torch.float32 else torch.int16
        assert torch.equal(zp.view(view), z_of.view(view))
        assert torch.equal(fan.hist[:, :, P - S:L - S].view(view), plain.hist[:, :, P:L].view(view))
        assert torch.equal(fan.tail, plain.tail)
        assert torch.equal(fan.hist[:, :, :P - S], below) and (shared is None or torch.equal(fan.hist_shared, shared))
        rows = [tuple(float(v) for v in fan.hist[b, 0, P - S:L - S].float().cpu()) for b in range(B)]
        assert len(set(rows)) > G                                               # (the rows of a group did diverge)


def case_state_refusals(dev):
    import pytest
    from hyena_dna_amd.hyena import HyenaOperator
    torch.manual_seed(0)
    op = HyenaOperator(d_model=8, **_layer(64)).to(dev).eval()
    par4 = torch.arange(4, dtype=torch.int32).to(dev)
    with pytest.raises(NotImplementedError, match="fan"):
        op.allocate_inference_cache(4, 32).reorder(par4)
    with pytest.raises(NotImplementedError, match="lookahead"):
        op.allocate_inference_cache(4, 32, lookahead=4).reorder(par4)
    st = op.allocate_inference_cache(4, 32, fan=2, prompt_len=8)
    for bad in (par4.long(), par4[:3], par4.tolist()):
        with pytest.raises(ValueError, match="parents"):
            st.reorder(bad)
    ragged = op.allocate_inference_cache(4, 32, fan=2, prompt_len=8)
    ragged.ragged = True
    with pytest.raises(NotImplementedError, match="ragged"):
        ragged.reorder(par4)


# ---- 4. the language model -------------------------------------------------------------------------------------------------------------------------
VOCAB = 12


def lm(dev, L, d=64, n_layer=2, seed=0):
    from hyena_dna_amd.lm import HyenaDNALM
    torch.manual_seed(seed)
    m = HyenaDNALM(d_model=d, n_layer=n_layer, d_inner=4 * d, vocab_size=VOCAB, layer=_layer(L + 2), resid_dropout=0.0, embed_dropout=0.1,
                   pad_vocab_size_multiple=8, fused_dropout_add_ln=True, residual_in_fp32=True)
    return m.to(dev).eval()


def prompts(G, P, dev, seed=4):
    return torch.randint(7, 11, (G, P), generator=torch.Generator().manual_seed(seed)).to(dev)


def gen(m, ids, N, **kw):
    kw.setdefault("use_cache", True)
    kw.setdefault("vocab_size", VOCAB)
    return m.generate(ids, max_length=ids.shape[1] + N, pad_token_id=PAD, return_dict_in_generate=True, **kw)


def teacher_forced(m, seq, P, N, tol=1e-5, stop=None):
    """seq (P + N,) -> (the fp64 sum of log-softmax over the live columns of the new tokens from ONE full forward, its tolerance, the
    per-token values); ``stop``: the tokens after the first ``stop`` do not count (a finished beam)"""
    with torch.no_grad():
        l64 = m(seq[None])[0].logits[0, P - 1:P + N - 1].float().cpu().double().numpy()
    toks = seq[P:P + N].cpu().numpy()
    lp, bd = DC.logprob_reference(l64, VOCAB, toks)
    total, bound, used = 0.0, 0.0, []
    for i in range(N):
        total += lp[i]
        bound += bd[i] + 1.01 * E32 * abs(total) + 2 * tol * np.abs(l64[i, :VOCAB]).max()
        used.append(lp[i])
        if stop is not None and toks[i] == stop:
            break
    return total, bound, np.array(used)


def case_lm_exhaustive(dev, seeds=(0, 1)):
    """k = 16, N = 2 over A C G T: the 16 returned sequences of a prompt are ALL 16 continuations, their scores the teacher-forced ones, the
    first the brute-force argmax wherever its lead exceeds the tolerance"""
    G, P, N, k = 2, 6, 2, 16
    decided = 0
    for seed in seeds:
        m = lm(dev, 40, seed=seed)
        ids = prompts(G, P, dev, seed=seed + 4)
        out = gen(m, ids, N, num_beams=k, num_return_sequences=k, allowed_tokens=ACGT)
        assert out._fields == ("sequences", "scores", "sequences_scores") and out.scores is None
        assert out.sequences.shape == (G * k, P + N) and out.sequences_scores.shape == (G * k,) and out.sequences_scores.dtype == torch.float32
        assert torch.equal(out.sequences[:, :P], ids.repeat_interleave(k, 0))
        for g in range(G):
            new = [tuple(r) for r in out.sequences[g * k:(g + 1) * k, P:].cpu().tolist()]
            assert sorted(new) == sorted((a, b) for a in ACGT for b in ACGT), new
            ref = []
            for r in range(k):
                want, tol, _ = teacher_forced(m, out.sequences[g * k + r], P, N)
                got = float(out.sequences_scores[g * k + r])
                assert abs(got - want) <= tol, (seed, g, r, got, want, tol)
                ref.append((want, tol))
            order = sorted(range(k), key=lambda r: -ref[r][0])
            if ref[order[0]][0] - ref[order[1]][0] > ref[order[0]][1] + ref[order[1]][1]:
                assert order[0] == 0, (seed, g, order[:3])
                decided += 1
            sc = out.sequences_scores[g * k:(g + 1) * k]
            assert bool((sc[:-1] >= sc[1:]).all())
    print(f"exhaustive search: the best beam decided in {decided} of {G * len(seeds)} prompts")
    assert decided == G * len(seeds)                                             # the seeds are chosen so that the top-2 gap exceeds the tolerance


def case_lm_pruning(dev, P=40, d=64, cg=False, autocast=None):
    """k = 4, N = 6, G = 2: every returned beam's score is its teacher-forced score, the scores descend, logprobs sum to the scores"""
    import contextlib
    G, N, k = 2, 6, 4
    m = lm(dev, P + N, d=d, seed=2)
    ids = prompts(G, P, dev)
    ctx = (lambda: torch.autocast("cuda", dtype=autocast)) if autocast is not None else contextlib.nullcontext
    with ctx():
        out = gen(m, ids, N, num_beams=k, num_return_sequences=k, allowed_tokens=ACGT, output_logprobs=True, cg=cg)
    assert out._fields == ("sequences", "scores", "sequences_scores", "logprobs") and out.logprobs.shape == (G * k, N)
    sc, lp = out.sequences_scores.cpu().double(), out.logprobs.cpu().double()
    toks = out.sequences[:, P:].cpu()
    assert bool(((toks >= 7) & (toks <= 10)).all())
    for g in range(G):
        assert bool((sc[g * k:(g + 1) * k][:-1] >= sc[g * k:(g + 1) * k][1:]).all())
        assert len(set(tuple(r) for r in toks[g * k:(g + 1) * k].tolist())) == k     # k different beams
    assert bool(((lp.sum(1) - sc).abs() <= N * 1.01 * E32 * lp.abs().sum(1)).all()), (lp.sum(1) - sc)
    worst = 0.0
    for r in range(G * k):
        with ctx():
            want, tol, each = teacher_forced(m, out.sequences[r], P, N, tol=1e-5 if autocast is None else 2e-2)
        worst = max(worst, abs(float(sc[r]) - want) / tol)
        assert abs(float(sc[r]) - want) <= tol, (r, float(sc[r]), want, tol)
    print(f"pruning search P={P} autocast={autocast}: worst |score - teacher forced| / tolerance = {worst:.4f}")
    return out


def case_lm_constraints(dev):
    from hyena_dna_amd.inference import iupac_constraints, token_mask
    m = lm(dev, 40)
    ids = prompts(2, 8, dev)
    c = iupac_constraints("ACGT").to(dev)
    out = gen(m, ids, 4, num_beams=2, num_return_sequences=2, constraints=c)
    assert out.sequences[0::2, 8:].cpu().tolist() == [ACGT, ACGT]                # rank 0: the one sequence the pattern leaves
    sc = out.sequences_scores.cpu()
    assert bool(torch.isfinite(sc[0::2]).all()) and bool((sc[1::2] == float("-inf")).all())
    for r in (0, 2):
        want, tol, _ = teacher_forced(m, out.sequences[r], 8, 4)
        assert abs(float(sc[r]) - want) <= tol
    pattern = "RYNA.S"
    rows = torch.stack([iupac_constraints(pattern), iupac_constraints("WWKMB.")]).to(dev)            # one row per prompt
    out = gen(m, ids, 6, num_beams=2, constraints=rows, allowed_tokens=ACGT + [11])
    assert out.sequences.shape == (2, 14)                                        # num_return_sequences = 1: the best beam of each prompt
    out = gen(m, ids, 6, num_beams=2, num_return_sequences=2, constraints=rows, allowed_tokens=ACGT + [11])
    keep = token_mask(ACGT + [11])
    for r in range(4):
        for i, t in enumerate(out.sequences[r, 8:].cpu().tolist()):
            assert (int(rows[r // 2, i]) & keep) >> t & 1, (r, i, t)


def case_lm_eos(dev):
    """a finished beam holds pad afterwards and keeps its score; stop_check_every ends early once every beam is finished"""
    from hyena_dna_amd.inference import token_mask
    G, P, N, k = 2, 8, 6, 4
    m = lm(dev, 40, seed=3)
    ids = prompts(G, P, dev)
    free = gen(m, ids, N, num_beams=k, num_return_sequences=k, allowed_tokens=ACGT)
    eos = int(free.sequences[0, P + 1])                                          # the best beam of prompt 0 emits it as its second token
    out = gen(m, ids, N, num_beams=k, num_return_sequences=k, allowed_tokens=ACGT, eos_token_id=eos, output_logprobs=True)
    toks = out.sequences[:, P:].cpu()
    finished = 0
    for r in range(G * k):
        hit = (toks[r] == eos).nonzero()
        stop = None
        if len(hit):
            finished += 1
            first = int(hit[0])
            assert bool((toks[r, first + 1:] == PAD).all()) and bool((out.logprobs[r, first + 1:] == 0).all())
            stop = eos
        want, tol, _ = teacher_forced(m, torch.where(out.sequences[r] == PAD, 7, out.sequences[r]), P, N, stop=stop)
        assert abs(float(out.sequences_scores[r]) - want) <= tol, (r, float(out.sequences_scores[r]), want)
    assert finished >= 1
    # every beam is forced to finish with its second token: the loop stops at the first check after it
    c = torch.full((N,), token_mask(ACGT), dtype=torch.int64)
    c[1] = token_mask([eos])
    c = c.to(dev)
    full = gen(m, ids, N, num_beams=k, num_return_sequences=k, constraints=c, eos_token_id=eos, output_logprobs=True)
    early = gen(m, ids, N, num_beams=k, num_return_sequences=k, constraints=c, eos_token_id=eos, output_logprobs=True, stop_check_every=1)
    assert full.logprobs.shape == (G * k, N) and early.logprobs.shape == (G * k, 2)
    assert torch.equal(early.sequences, full.sequences) and torch.equal(early.sequences_scores, full.sequences_scores)
    assert torch.equal(early.logprobs, full.logprobs[:, :2]) and bool((full.sequences[:, P + 2:] == PAD).all())
    # min_new_tokens holds eos back
    out = gen(m, ids, N, num_beams=k, num_return_sequences=k, allowed_tokens=ACGT, eos_token_id=eos, min_new_tokens=3)
    assert bool((out.sequences[:, P:P + 3] != eos).all())


def case_lm_one_beam_is_todays_generate(dev):
    m = lm(dev, 40)
    ids = prompts(3, 8, dev)
    for kw in (dict(), dict(use_cache=True), dict(use_cache=True, sampler="device", top_k=4, seed=3, num_return_sequences=2, output_logprobs=True)):
        kw = dict(kw, max_length=14, return_dict_in_generate=True)
        ref = m.generate(ids, **kw)
        for nb in (None, 1):
            out = m.generate(ids, num_beams=nb, **kw)
            assert out._fields == ref._fields and torch.equal(out.sequences, ref.sequences)
            if "logprobs" in ref._fields:
                assert torch.equal(out.logprobs, ref.logprobs)
    assert torch.equal(m.generate(ids, max_length=8, use_cache=True, num_beams=2), ids)              # nothing to generate
    assert m.generate(ids, max_length=8, use_cache=True, num_beams=3, num_return_sequences=2).shape == (6, 8)


def case_lm_refusals(dev):
    """every refusal of generate(num_beams=k), each before a cache exists"""
    import pytest
    m = lm(dev, 40)
    ids = prompts(2, 8, dev)

    def no_cache(*a, **kw):
        raise AssertionError("a cache was built before the refusal")
    m.allocate_inference_cache = no_cache
    ok = dict(max_length=12, use_cache=True, num_beams=4)
    for kw, exc, match in ((dict(use_cache=False), ValueError, "use_cache"), (dict(sampler="torch"), ValueError, "sampler"),
                           (dict(top_k=2), ValueError, "top_k"), (dict(top_p=0.9), ValueError, "top_p"),
                           (dict(temperature=0.7), ValueError, "temperature"), (dict(seed=1), ValueError, "seed"),
                           (dict(output_scores=True), ValueError, "output_scores"),
                           (dict(lengths=torch.tensor([8, 5], dtype=torch.int32).to(dev)), NotImplementedError, "ragged"),
                           (dict(lookahead=4), NotImplementedError, "lookahead"), (dict(num_return_sequences=5), ValueError, "num_return_sequences"),
                           (dict(num_return_sequences=0), ValueError, "num_return_sequences"), (dict(num_beams=17), ValueError, "num_beams"),
                           (dict(num_beams=0), ValueError, "num_beams"), (dict(num_beams=-2), ValueError, "num_beams"),
                           (dict(vocab_size=17), ValueError, "vocab_size"), (dict(allowed_tokens=[12, 13], vocab_size=12), ValueError, "allow no token"),
                           (dict(min_new_tokens=2), ValueError, "eos_token_id")):
        with pytest.raises(exc, match=match):
            m.generate(ids, **dict(ok, **kw))
    with pytest.raises(AssertionError, match="a cache was built"):               # (the good call does get that far)
        m.generate(ids, **ok)
    from hyena_dna_amd.lm import HyenaDNALM
    torch.manual_seed(0)
    wide = HyenaDNALM(d_model=64, n_layer=1, d_inner=256, vocab_size=70, layer=_layer(42), resid_dropout=0.0, embed_dropout=0.1,
                      pad_vocab_size_multiple=8, fused_dropout_add_ln=True, residual_in_fp32=True).to(dev).eval()
    wide.allocate_inference_cache = no_cache
    with pytest.raises(ValueError, match="64 columns"):
        wide.generate(ids, **ok)
    del m.allocate_inference_cache
    ip_like = type("IP", (), {})()
    ip_like.key_value_memory_dict = m.allocate_inference_cache(4, 12)
    with pytest.raises(NotImplementedError, match="fan"):
        m.reorder_inference_cache(ip_like, torch.arange(4, dtype=torch.int32).to(dev))


def manual_search(m, ids, k, N, cg, eos=None):
    """generate(num_beams=k, allowed_tokens=ACGT)'s loop by hand, so that the caches and the searcher can be looked at afterwards"""
    from hyena_dna_amd.inference import BeamSearcher, InferenceParams, token_mask
    from hyena_dna_amd.lm import GraphedDecodeStep
    G, P = ids.shape
    B = G * k
    allow = torch.full((N,), token_mask(ACGT), dtype=torch.int64).to(ids.device)
    with torch.no_grad():
        ip = InferenceParams(max_seqlen=P + N, max_batch_size=B)
        ip.key_value_memory_dict = m.allocate_inference_cache(B, P + N, fan=k, prompt_len=P)
        last = m(ids, inference_params=ip)[0].logits[:, -1].repeat_interleave(k, 0)
        search = BeamSearcher(ip.key_value_memory_dict.values(), ids, k, N, eos=eos, pad=PAD, vocab=VOCAB, allow=allow)
        ip.seqlen_offset = P
        step = GraphedDecodeStep(m, ip, B, sampler=search) if cg else None
        nxt = step.ids if cg else torch.empty(B, 1, dtype=torch.int64, device=ids.device)
        search(last, nxt)
        for i in range(1, N):
            if cg:
                step.replay()
            else:
                search(m(nxt, inference_params=ip)[0].logits[:, -1], nxt)
            ip.seqlen_offset += 1
        if cg:
            step.release()
    return search, list(ip.key_value_memory_dict.values()), nxt.clone()


def case_lm_graph_equals_eager(dev, P=40, d=64):
    """cg=True against the eager path bit for bit -- sequences, sequences_scores, logprobs -- and, after release(), the caches' tail / pos /
    history columns and the searcher's state"""
    G, N, k = 2, 6, 4
    m = lm(dev, P + N, d=d, seed=2)
    ids = prompts(G, P, dev)
    kw = dict(num_beams=k, num_return_sequences=3, allowed_tokens=ACGT, output_logprobs=True)
    a, b = gen(m, ids, N, **kw), gen(m, ids, N, cg=True, **kw)
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.sequences_scores.view(torch.int32), b.sequences_scores.view(torch.int32))
    assert torch.equal(a.logprobs.view(torch.int32), b.logprobs.view(torch.int32))
    (se, ce, ne), (sg, cgs, ng) = manual_search(m, ids, k, N, False), manual_search(m, ids, k, N, True)
    assert torch.equal(ne, ng)
    for name in ("score", "col", "done", "parent", "tok_hist", "parent_hist", "lp_hist"):
        x, y = getattr(se, name), getattr(sg, name)
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name
    for x, y in zip(ce, cgs):
        assert torch.equal(x.tail, y.tail) and torch.equal(x.pos, y.pos) and x.pos.item() == P + N - 1
        assert torch.equal(x.hist[:, :, :P + N - 1 - x.S], y.hist[:, :, :P + N - 1 - x.S])
    seq, sc, lp = sg.finalize(N, 3, want_logprobs=True)
    assert torch.equal(seq, a.sequences) and torch.equal(sc, a.sequences_scores) and torch.equal(lp.view(torch.int32), a.logprobs.view(torch.int32))
