"""Automaton-constrained generation -- inference.TokenAutomaton / motif_automaton / automaton_step_tables, csrc/decode_kernels.h
decode_sample_con_kernel and decode_beam_kernel in their AUTO instantiations, include/hyena_decode.h hyena_decode_sample_automaton /
hyena_decode_beam_automaton, generate(automaton=...) -- held to plain-Python restatements.  The cases live here and run twice: under
tests/hipemu on the CPU (test_decode_automaton_emu.py, which also runs the host-only cases) and on the gfx950 binary
(test_gpu_decode_automaton.py).

Every comparison is exact.  The new kernels share their bodies with the constrained sampler and the beam kernel, so
  * the sampler is held (a) bit for bit, every output, to hyena_decode_sample_constrained fed with the masks looked up from M at the states
    this module tracks with delta itself, and (b) to decode_constrain_local's fp64 restatement on those masks (tokens outside its own
    "left out" draws; log-probs within its BOUND);
  * the beam kernel is held to decode_beam_local.check_beam with the allowed sets taken from M, and dstate to delta[state[parent], tok];
  * the language-model cases replay a constrained run through generate(constraints=...) -- the existing kernel -- with torch.equal."""
import itertools
import re

import numpy as np
import torch

from tests import decode_beam_local as DB
from tests import decode_constrain_local as DC
from tests import decode_sample_local as DS

SEED, NCOLS = DS.SEED, DS.NCOLS
SHAPES, DTYPES = DC.SHAPES, DC.DTYPES
ACGT = DC.ACGT
BASES = "ACGT"
TOK = dict(zip(BASES, ACGT))
LETTER = {v: k for k, v in TOK.items()}
OTHER = 11                                                                       # 'N' of the character tokenizer: not one of the four bases
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "R": "Y", "Y": "R", "S": "S", "W": "W", "K": "M", "M": "K", "B": "V", "V": "B", "D": "H",
        "H": "D", "N": "N"}


# ---- 1. host: motif_automaton against brute force ------------------------------------------------------------------------------------------------
def _regex(motif):
    from hyena_dna_amd.inference import IUPAC
    return re.compile("".join("[" + IUPAC[ch] + "]" for ch in motif))


def _revcomp(motif):
    return "".join(COMP[ch] for ch in reversed(motif))


def brute_force(s, avoid, require, h, rc):
    """s: a string over ACGT and 'x' (any other token) -> (no avoided motif and no run longer than h anywhere, every required motif occurs).
    Motifs are searched in the maximal runs of bases: another token breaks every motif and every run."""
    parts = s.split("x")
    av = [m for m in avoid] + ([_revcomp(m) for m in avoid] if rc else [])
    clean = not any(_regex(m).search(p) for m in av for p in parts)
    if h is not None:
        clean = clean and not any(re.search(r"(.)\1{%d}" % h, p) for p in parts)
    seen = all(any(_regex(v).search(p) for p in parts for v in ([m, _revcomp(m)] if rc else [m])) for m in require)
    return clean, seen


MOTIF_CASES = [dict(avoid=["GAATTC"]), dict(avoid=["GAATTC"], reverse_complement=True), dict(avoid=["GGTCTC"]),
               dict(avoid=["GGTCTC"], reverse_complement=True), dict(max_homopolymer=1), dict(max_homopolymer=3),
               dict(avoid=["GRY", "TTNA"], max_homopolymer=3, reverse_complement=True), dict(require=["TATA", "ATAC"]),
               dict(require=["TATA", "ATAC"], avoid=["CG"], max_homopolymer=2, reverse_complement=True)]
WITH_OTHER = ["GAAxTTC", "GAATTxC", "xGAATTC", "GAATTCx", "AAAxAAA", "AxA", "TATxA", "TATAxATAC", "TATxATAC", "ATACxxTATA", "GGTCxTC", "GAGACCx",
              "GxAC", "GAxC", "TTGAx", "x", "xx", "TATACx", "xTATAC"]


def case_motif_vs_brute_force(kw, max_len=8):
    from hyena_dna_amd.inference import motif_automaton
    A = motif_automaton(**kw)
    avoid, require = kw.get("avoid", ()), kw.get("require", ())
    h, rc = kw.get("max_homopolymer"), kw.get("reverse_complement", False)
    longest = max([len(m) for m in list(avoid) + list(require)], default=1)
    assert A.context == max(longest - 1, h or 0) and A.start == 0 and A.V == 16
    delta, accept = A.delta.tolist(), A.accept.tolist()
    col = dict(TOK, x=OTHER)
    n = 0
    strings = ("".join(t) for L in range(max_len + 1) for t in itertools.product(BASES, repeat=L))
    for s in itertools.chain(strings, WITH_OTHER):
        st = 0
        for ch in s:
            st = delta[st][col[ch]]
            if st < 0:
                break
        clean, seen = brute_force(s, avoid, require, h, rc)
        assert (st >= 0) == clean, (kw, s)
        if st >= 0:
            assert accept[st] == seen, (kw, s)
        n += 1
    # the other tokens all behave as one, and the public walk agrees with the table
    assert all(row[OTHER] == row[v] for row in delta for v in range(16) if v not in ACGT)
    site, st, want = [TOK[c] for c in "GAATTCA"], 0, []
    for v in site:
        st = delta[st][v] if st >= 0 else -1
        want.append(st)
    assert A.walk(site) == want and A.accepts(site) == (want[-1] >= 0 and accept[want[-1]])
    print(f"{kw}: {A.S} states, {n} strings")
    return A


def case_motif_limits():
    import pytest
    from hyena_dna_amd.inference import TokenAutomaton, motif_automaton
    many = ["".join(t) for t in itertools.product(BASES, repeat=3)][5:18]       # 13 required motifs: 2^13 sets of seen bits
    with pytest.raises(ValueError, match="more than 4096"):
        motif_automaton(require=many)
    for bad in (dict(avoid=["GAXT"]), dict(avoid=[""]), dict(max_homopolymer=0), dict(n_tokens=65), dict(n_tokens=8),
                dict(token_of=dict(A=1, C=1, G=2, T=3))):
        with pytest.raises(ValueError):
            motif_automaton(**bad)
    other = motif_automaton(avoid=["AC"], token_of=dict(A=0, C=1, G=2, T=3), n_tokens=4)
    assert other.V == 4 and other.walk([0, 1]) [-1] == -1 and other.walk([0, 2, 1])[-1] >= 0
    ok = torch.zeros(2, 4, dtype=torch.int32)
    for bad in (dict(delta=ok.long()), dict(delta=ok[0]), dict(delta=ok.tolist()), dict(delta=torch.zeros(4097, 4, dtype=torch.int32)),
                dict(delta=torch.zeros(2, 65, dtype=torch.int32)), dict(delta=ok + 2), dict(delta=ok - 2), dict(delta=ok, accept=torch.ones(3, dtype=torch.bool)),
                dict(delta=ok, accept=torch.ones(2)), dict(delta=ok, start=2), dict(delta=ok, start=-1), dict(delta=ok, context=-1)):
        with pytest.raises(ValueError):
            TokenAutomaton(**bad)
    A = TokenAutomaton(ok, context=3)
    assert A.S == 2 and A.V == 4 and bool(A.accept.all()) and A.accepts([0, 1, 2]) and A.initial_state([1, 2]) == 0


# ---- 2. host: the step tables against exhaustive enumeration --------------------------------------------------------------------------------------
EOS = 1


def exists_completion(A, delta, accept, i, s, N, P, eos):
    """plain recursion over every continuation: can positions i .. N - 1 be filled from state s so that the word is accepted?"""
    if i == N:
        return accept[s]
    for v in P[i]:
        if v == eos:
            if accept[s]:
                return True
        elif delta[s][v] >= 0 and exists_completion(A, delta, accept, i + 1, delta[s][v], N, P, eos):
            return True
    return False


def case_tables_vs_enumeration(kw, N, pattern, eos, m):
    """bit v of M[i][s] is set exactly when token v at position i in state s leaves a completion"""
    from hyena_dna_amd.inference import automaton_step_tables, iupac_constraints, motif_automaton, token_mask
    A = motif_automaton(**kw)
    keep = token_mask(ACGT + ([eos] if eos is not None else []))
    masks = iupac_constraints(pattern) & keep
    assert len(masks) == N
    if m and eos is not None:
        masks[:m] &= ~token_mask([eos])
    M = automaton_step_tables(A, N, masks=masks, eos=eos, vocab=12)
    assert M.shape == (N, A.S) and M.dtype == torch.int64
    delta, accept = A.delta.tolist(), A.accept.tolist()
    P = [[v for v in range(12) if (int(x) >> v) & 1] for x in masks.tolist()]
    for i in range(N):
        for s in range(A.S):
            want = 0
            for v in P[i]:
                if v == eos:
                    good = accept[s]
                else:
                    good = delta[s][v] >= 0 and exists_completion(A, delta, accept, i + 1, delta[s][v], N, P, eos)
                want |= (1 << v) if good else 0
            assert int(M[i, s]) == want, (kw, i, s, int(M[i, s]), want)
    return A, M


TABLE_CASES = [(dict(avoid=["AA", "CG"], max_homopolymer=2), 6, "N.N.NN", EOS, 2),
               (dict(avoid=["GAT"], require=["TA"]), 6, "......", None, 0),
               (dict(require=["ACA", "CAC"]), 5, "NNNNN", EOS, 0),
               (dict(avoid=["AC"], reverse_complement=True, require=["GG"]), 6, "RNYN.N", EOS, 3),
               (dict(max_homopolymer=1), 4, "WWSS", None, 0)]


def case_tables_position_independent():
    """Nt == 1 exactly where nothing depends on the position; there M[0] prunes the transitions into states without an infinite
    continuation, and nothing else"""
    from hyena_dna_amd.inference import TokenAutomaton, automaton_step_tables, iupac_constraints, motif_automaton, token_mask
    from hyena_dna_amd.lm import _automaton_tables
    ids = torch.tensor([[7, 8, 9, 10, 7, 7]])
    plain, req = motif_automaton(avoid=["GAATTC"], max_homopolymer=3), motif_automaton(require=["TATA"])
    N = 8
    pat = iupac_constraints("N" * N)

    def nt(A, **kw):
        a = dict(allowed_tokens=None, constraints=None, min_new_tokens=0, eos_token_id=None)
        a.update(kw)
        M, delta, dstate = _automaton_tables(A, ids, None, 1, N, 16, 12, a["allowed_tokens"], a["constraints"], a["min_new_tokens"], a["eos_token_id"])
        assert M.shape[1] == A.S and delta.shape == (A.S, 16) and dstate.shape == (1,)
        return M.shape[0]

    assert nt(plain) == 1 and nt(plain, allowed_tokens=ACGT) == 1 and nt(plain, eos_token_id=EOS) == 1
    assert nt(plain, allowed_tokens=ACGT + [EOS], eos_token_id=EOS) == 1
    assert nt(plain, constraints=pat) == N and nt(plain, eos_token_id=EOS, min_new_tokens=1) == N and nt(req) == N
    assert nt(req, allowed_tokens=ACGT, eos_token_id=EOS) == N
    # a hand-made dead end: 0 -A-> 1, 1 has no way on; 0 -C-> 0; 0 -G-> 2 -G-> 2.  Token 3 is forbidden everywhere.
    delta = torch.full((3, 4), -1, dtype=torch.int32)
    delta[0, 0], delta[0, 1], delta[0, 2], delta[2, 2] = 1, 0, 2, 2
    A = TokenAutomaton(delta)
    M1 = automaton_step_tables(A, 5)
    assert M1.shape == (1, 3) and M1[0].tolist() == [0b110, 0, 0b100]          # A is pruned although delta allows it; state 1 is dead
    MN = automaton_step_tables(A, 5, positional=True)
    assert MN.shape == (5, 3) and MN[4].tolist() == [0b111, 0, 0b100] and MN[3].tolist() == [0b110, 0, 0b100]   # (the last token may step into the dead end)
    ME = automaton_step_tables(A, 5, eos=3)                                      # with eos every state can end: nothing is pruned
    assert ME.shape == (1, 3) and ME[0].tolist() == [0b1111, 0b1000, 0b1100]
    # the motif automaton: where only A may be emitted and runs of A are capped, every state is dead
    M = automaton_step_tables(motif_automaton(max_homopolymer=2), 6, masks=torch.full((6,), token_mask([7])), positional=False)
    assert M.shape[0] == 1 and bool((M == 0).all())
    # the fixed point agrees with the backward pass far from the end
    for A in (plain, motif_automaton(avoid=["AC", "CA", "AA"], max_homopolymer=1)):
        keep = torch.full((A.S + 3,), token_mask(ACGT))
        assert torch.equal(automaton_step_tables(A, A.S + 3, masks=keep, vocab=12, positional=False)[0],
                           automaton_step_tables(A, A.S + 3, masks=keep, vocab=12, positional=True)[0])
    import pytest
    big = TokenAutomaton(torch.zeros(4096, 4, dtype=torch.int32), accept=torch.arange(4096) > 0)
    with pytest.raises(ValueError, match="2\\^22"):
        automaton_step_tables(big, 1025)
    assert automaton_step_tables(big, 1024).shape == (1024, 4096)


# ---- 3. the sampler kernel -----------------------------------------------------------------------------------------------------------------------
def random_automaton(S, V, Nt, seed, zero_rows=True):
    """-> delta (S, V) int32 with some -1, M (Nt, S) uint64 random masks (a few empty, a few with dead bits only)"""
    rng = np.random.default_rng(seed)
    delta = rng.integers(-1, S, size=(S, V)).astype(np.int32)
    M = rng.integers(0, 2 ** 64, size=(Nt, S), dtype=np.uint64) & rng.integers(0, 2 ** 64, size=(Nt, S), dtype=np.uint64)
    if zero_rows:
        M[rng.integers(0, Nt), rng.integers(0, S)] = 0
        M[rng.integers(0, Nt), rng.integers(0, S)] = np.uint64(1) << np.uint64(63)
    return delta, M


def lookup_masks(M, state, n, S):
    """the header's rule -> uint64 (B,): M[(Nt == 1 ? 0 : n), s], 0 (no mask: the whole live vocabulary) for s outside [0, S) or n outside"""
    Nt = M.shape[0]
    inside = (state >= 0) & (state < S) & ((Nt == 1) | ((n >= 0) & (n < Nt)))
    row = np.zeros_like(n) if Nt == 1 else np.clip(n, 0, Nt - 1)
    return np.where(inside, M[row, np.clip(state, 0, S - 1)], np.uint64(0))


def run_auto(_lib, dev, logits, col, done, start, dstate, M, delta, T, top_k, top_p, Vlive, eos, pad, ldp=NCOLS):
    """one call of hyena_decode_sample_automaton on copies of the state and sentinel-filled outputs -> dict of CPU tensors"""
    B, V = logits.shape
    o = dict(seq=torch.full((B, NCOLS), -7, dtype=torch.int64), nxt=torch.full((B, 1), -9, dtype=torch.int64), col=col.clone(),
             done=done.clone(), scores=torch.full((B, NCOLS, V), float("nan")), u=torch.full((B,), float("nan")),
             lp=torch.full((B, ldp), -777.0), dstate=dstate.clone())
    o = {k: v.to(dev) for k, v in o.items()}
    _lib.decode_sample(logits.to(dev), DS.seed_tensor(SEED, dev), o["col"], o["done"], o["seq"], o["nxt"], temperature=T, top_k=top_k, top_p=top_p,
                       eos=eos, pad=pad, vocab=Vlive, scores=o["scores"], u_out=o["u"], start=start.to(dev), logprobs=o["lp"],
                       automaton=(DC.masks_to_tensor(M).to(dev), torch.from_numpy(delta).to(dev), o["dstate"]))
    o = {k: v.cpu() for k, v in o.items()}
    o["nxt"] = o["nxt"][:, 0]
    return o


def same_outputs(a, b, what):
    DC.same_bits(a, b)
    assert torch.equal(a["lp"].view(torch.int32), b["lp"].view(torch.int32)), what


def case_sampler(_lib, dev, V, Vlive, dtype, B=24, calls=4):
    """consecutive calls on random logits; rows in different states, parked on either side, done, and with states outside the table"""
    S, Nt, eos, pad = 5, 3, 2, 1
    delta, M = random_automaton(S, V, Nt, 11 * V + Vlive)
    g = torch.Generator().manual_seed(V + Vlive)
    col = torch.randint(0, 3, (B,), generator=g, dtype=torch.int32)
    start = torch.randint(0, 2, (B,), generator=g, dtype=torch.int32)            # n = col - start: -1 ... 2, then it grows past Nt
    col[3], col[7] = -1, NCOLS                                                   # parked
    done = torch.zeros(B, dtype=torch.int32)
    done[5] = 1
    state = torch.randint(0, S, (B,), generator=g, dtype=torch.int32)
    state[9], state[10] = -3, S                                                  # outside the table: unmasked, and the state stays
    live = np.arange(V) < Vlive
    left = checked = 0
    for step in range(calls):
        for top_k, top_p, T in ((1, 1.0, 1.0), (4, 0.9, 0.7), (V, 0.3, 1.0))[step % 3:step % 3 + 1]:
            logits = (torch.randn(B, V, generator=g) * 2.0).to(dtype)
            if step == 2:
                logits[0] = float("nan")                                         # the kernel stays total
            n = (col - start).numpy().astype(np.int64)
            masks = lookup_masks(M, state.numpy(), n, S)
            out = run_auto(_lib, dev, logits, col, done, start, state, M, delta, T, top_k, top_p, Vlive, eos, pad)
            # (a) the existing kernel on the looked-up masks: one mask per row, n forced to 0 by start = col
            allow = DC.masks_to_tensor(masks[:, None])
            ref = DC.run_kernel(_lib, dev, logits, col, SEED, T, top_k, top_p, Vlive, eos=eos, pad=pad, done=done, allow=allow, start=col.clamp(0, NCOLS),
                                want_logprobs=True)
            for k in ("seq", "nxt", "col", "done"):
                assert torch.equal(out[k], ref[k]), (k, step)
            for k in ("scores", "u"):
                assert torch.equal(out[k].view(torch.int32), ref[k].view(torch.int32)), (k, step)
            act = ((col >= 0) & (col < NCOLS) & (done == 0)).numpy()
            rows = np.nonzero(act)[0]
            tok = out["seq"][rows, col[rows].long()].numpy()
            slot = (n[rows] >= 0) & (n[rows] < NCOLS)
            assert torch.equal(out["lp"][rows[slot], n[rows][slot]].view(torch.int32), ref["lp"][rows[slot], 0].view(torch.int32)), step
            assert int((out["lp"] != -777.0).sum()) == int(slot.sum())
            # (b) the fp64 restatement on the same sets
            A = np.tile(live, (B, 1))
            mb = DC.bits(masks, V) & live[None]
            A[mb.any(1)] = mb[mb.any(1)]
            u = DS.uniforms(SEED, B, NCOLS)[np.arange(B), col.clamp(0, NCOLS - 1).numpy()]
            l64 = logits.double().numpy()
            want, left_out = DC.reference(l64[rows], A[rows], Vlive, float(np.float32(T)), top_k, float(np.float32(top_p)), u[rows])
            assert bool(A[rows, tok].all())
            assert (tok[~left_out] == want[~left_out]).all(), (step, tok, want)
            left, checked = left + int(left_out.sum()), checked + len(rows)
            lp, bound = DC.logprob_reference(l64[rows[slot]], Vlive, tok[slot])
            DC.check_logprobs(out["lp"][rows[slot], n[rows][slot]], lp, bound, ("lp", step))
            # the state: delta[s, tok], unless eos, a forbidden token (through the fall-back), a state outside the table; other rows keep theirs
            want_state = state.clone()
            for r, t in zip(rows, tok):
                s = int(state[r])
                if 0 <= s < S and t != eos and delta[s, t] >= 0:
                    want_state[r] = int(delta[s, t])
            assert torch.equal(out["dstate"], want_state), (step, out["dstate"].tolist(), want_state.tolist())
            assert out["dstate"][9] == -3 and out["dstate"][10] == S and out["col"][3] == -1 and out["nxt"][3] == -9 and out["nxt"][5] == pad
            col, done, state = out["col"], out["done"], out["dstate"]
    assert left <= 0.02 * checked + 1, (left, checked)
    return checked


def case_sampler_grid_stride(_lib, dev, dtype):
    """more rows than workgroups (the size of decode_sample_local.case_nonfinite_grid_stride): row b + 2^16 runs after row b in one
    workgroup, each in its own state"""
    V, Vlive, n = 16, 12, DS.B_CASE
    B = DS.SMP_MAX_GRID + n
    S, Nt = 7, 1
    delta, M = random_automaton(S, V, Nt, 5)
    base = DS.make_logits(V, Vlive, dtype, 7)
    logits = torch.zeros(B, V, dtype=dtype)
    logits[:n], logits[DS.SMP_MAX_GRID:] = DS.plant_nonfinite(base, Vlive), base
    col = torch.full((B,), -1, dtype=torch.int32)
    col[:n], col[DS.SMP_MAX_GRID:] = 5, 2
    state = (torch.arange(B) % (S + 1)).int()                                   # (some rows at S: outside)
    zeros = torch.zeros(B, dtype=torch.int32)
    out = run_auto(_lib, dev, logits, col, zeros, zeros, state, M, delta, 0.7, 4, 0.9, Vlive, 3, 0)
    masks = lookup_masks(M, state.numpy(), col.numpy().astype(np.int64), S)
    ref = DC.run_kernel(_lib, dev, logits, col, SEED, 0.7, 4, 0.9, Vlive, eos=3, pad=0, allow=DC.masks_to_tensor(masks[:, None]), start=col.clamp(0, NCOLS),
                        want_logprobs=True)
    for k in ("seq", "nxt", "col", "done"):
        assert torch.equal(out[k], ref[k]), k
    assert torch.equal(out["u"].view(torch.int32), ref["u"].view(torch.int32))
    act = (col >= 0).numpy()
    tok = out["seq"][np.nonzero(act)[0], col[act].long()].numpy()
    want = state.clone()
    for r, t in zip(np.nonzero(act)[0], tok):
        s = int(state[r])
        if s < S and t != 3 and delta[s, t] >= 0:
            want[r] = int(delta[s, t])
    assert torch.equal(out["dstate"], want) and bool((out["seq"][n:DS.SMP_MAX_GRID] == -7).all())


def case_degenerate(_lib, dev, V, Vlive, dtype):
    """S = 1, delta == 0, M an (N,) row of masks: hyena_decode_sample_constrained bit for bit; all-ones masks: hyena_decode_sample"""
    base = DS.make_logits(V, Vlive, dtype, 100 + V + Vlive)
    B = DS.B_CASE
    col = DS.make_cols(V + Vlive)
    done = (torch.arange(B) % 11 == 3).int()
    start = torch.from_numpy(np.random.default_rng(V).integers(0, 3, size=B).astype(np.int32))
    delta = np.zeros((1, V), dtype=np.int32)
    rand = np.random.default_rng(7 + V).integers(0, 2 ** 64, size=(NCOLS, 1), dtype=np.uint64)
    rand[2] = 0                                                                  # an empty mask: the whole live vocabulary in both kernels
    ones = np.full((NCOLS, 1), 2 ** 64 - 1, dtype=np.uint64)
    zeros = torch.zeros(B, dtype=torch.int32)
    for logits in (base, DS.plant_nonfinite(base, Vlive)):
        for top_k, top_p, T in ((1, 1.0, 1.0), (4, 0.9, 0.7), (V, 0.3, 1.0)):
            kw = dict(eos=3, pad=5, done=done)
            got = run_auto(_lib, dev, logits, col, done, start, zeros, rand, delta, T, top_k, top_p, Vlive, 3, 5)
            con = DC.run_kernel(_lib, dev, logits, col, SEED, T, top_k, top_p, Vlive, allow=DC.masks_to_tensor(rand[:, 0]), start=start,
                                want_logprobs=True, **kw)
            same_outputs(got, con, (top_k, top_p, T))
            assert bool((got["dstate"] == 0).all())
            got = run_auto(_lib, dev, logits, col, done, start, zeros, ones, delta, T, top_k, top_p, Vlive, 3, 5)
            DC.same_bits(got, DC.run_kernel(_lib, dev, logits, col, SEED, T, top_k, top_p, Vlive, old=True, **kw))
            got = run_auto(_lib, dev, logits, col, done, start, zeros, ones[:1], delta, T, top_k, top_p, Vlive, 3, 5)      # Nt == 1
            DC.same_bits(got, DC.run_kernel(_lib, dev, logits, col, SEED, T, top_k, top_p, Vlive, old=True, **kw))


# ---- 4. the beam kernel --------------------------------------------------------------------------------------------------------------------------
BEAM_KS, BEAM_GS = (1, 3, 16), (1, 3)


def run_beam_auto(_lib, dev, logits, score, done, col, start, dstate, M, delta, k, Vlive, eos, pad, nrec=6):
    B = logits.shape[0]
    o = dict(score=score.clone(), done=done.clone(), col=col.clone(), parent=torch.full((B,), -5, dtype=torch.int32),
             nxt=torch.full((B, 1), -9, dtype=torch.int64), tok_hist=torch.full((B, nrec), -3, dtype=torch.int32),
             parent_hist=torch.full((B, nrec), -4, dtype=torch.int32), lp_hist=torch.full((B, nrec), -777.0), dstate=dstate.clone())
    o = {n: t.to(dev) for n, t in o.items()}
    _lib.decode_beam(logits.to(dev), o["score"], o["col"], o["done"], start.to(dev), o["parent"], o["nxt"], k, DB.NCOLS, eos=eos, pad=pad, vocab=Vlive,
                     tok_hist=o["tok_hist"], parent_hist=o["parent_hist"], lp_hist=o["lp_hist"],
                     automaton=(DC.masks_to_tensor(M).to(dev), torch.from_numpy(delta).to(dev), o["dstate"]))
    o = {n: t.cpu() for n, t in o.items()}
    o["nxt"] = o["nxt"][:, 0]
    return o


def case_beam(_lib, dev, V, Vlive, dtype, steps=3):
    """several steps fed forward, the allowed sets from M at the tracked states; a step of constant logits (ties), finished beams, a parked
    group, a state outside the table"""
    stats = dict(groups=0, undecided=0)
    live = np.arange(V) < Vlive
    for k in BEAM_KS:
        for G in BEAM_GS:
            B = G * k
            S, Nt, pad = 6, (1, 4)[k % 2], 1
            delta, M = random_automaton(S, V, Nt, 100 * k + G + V)
            g = torch.Generator().manual_seed(1000 * V + 10 * Vlive + k + G)
            score = torch.full((G, k), float("-inf"))
            score[:, 0] = 0.0
            score = score.reshape(B)
            done = torch.zeros(B, dtype=torch.int32)
            col = torch.full((B,), 2, dtype=torch.int32)
            start = torch.full((B,), 2, dtype=torch.int32)
            if G > 1:
                col[k:2 * k] = DB.NCOLS                                          # a parked group
            state = torch.randint(0, S, (B,), generator=g, dtype=torch.int32)
            if B > 2:
                state[B - 1] = S + 2
            for step in range(steps):
                logits = (torch.randn(B, V, generator=g) * 2.0).to(dtype)
                if step == 1:
                    logits[:k] = 0.75                                            # group 0: ties within every row
                    if k > 1:
                        done[1] = 1                                              # ... and a finished beam
                eos = int(logits[B - 1, :Vlive].float().argmax())
                n = (col - start).numpy().astype(np.int64)
                masks = lookup_masks(M, state.numpy(), n, S)
                A = np.tile(live, (B, 1))
                mb = DC.bits(masks, V) & live[None]
                A[mb.any(1)] = mb[mb.any(1)]
                o = run_beam_auto(_lib, dev, logits, score, done, col, start, state, M, delta, k, Vlive, eos, pad)
                DB.check_beam(o, logits, score, done, col, start, A, k, Vlive, eos, pad, 6, stats)
                want = state.clone()
                for b in range(B):
                    if not 0 <= int(col[b // k * k]) < DB.NCOLS:
                        continue
                    p, t = int(o["parent"][b]), int(o["nxt"][b])
                    s = int(state[p])
                    want[b] = s
                    if not done[p] and t != eos and 0 <= s < S and delta[s, t] >= 0:
                        want[b] = int(delta[s, t])
                assert torch.equal(o["dstate"], want), (k, G, step, o["dstate"].tolist(), want.tolist())
                score, done, col, state = o["score"], o["done"], o["col"], o["dstate"]
    assert stats["undecided"] * 100 <= stats["groups"] + 100
    return stats


# ---- 5. the C entry points' refusals ---------------------------------------------------------------------------------------------------------------
def case_abi_refusals(_lib, dev):
    import ctypes
    L = _lib.lib()
    B, V, ncols, S, Nt, fan = 4, 16, 8, 3, 2, 2
    t = dict(logits=torch.zeros(B, V), seed=torch.zeros(1, dtype=torch.int64), col=torch.zeros(B, dtype=torch.int32),
             done=torch.zeros(B, dtype=torch.int32), seq=torch.zeros(B, ncols, dtype=torch.int64), nxt=torch.zeros(B, dtype=torch.int64),
             M=torch.full((Nt, S), -1, dtype=torch.int64), delta=torch.ones(S, V, dtype=torch.int32), dstate=torch.zeros(B, dtype=torch.int32),
             start=torch.zeros(B, dtype=torch.int32), lp=torch.zeros(B, ncols), score=torch.zeros(B), parent=torch.full((B,), -5, dtype=torch.int32),
             th=torch.zeros(B, ncols, dtype=torch.int32), ph=torch.zeros(B, ncols, dtype=torch.int32), lh=torch.zeros(B, ncols))
    t = {k: v.to(dev) for k, v in t.items()}
    p = {k: v.data_ptr() for k, v in t.items()}

    def sample(**kw):
        a = dict(p, ldl=V, dtype=0, B=B, V=V, Vlive=12, T=1.0, top_k=4, top_p=0.9, eos=-1, pad=0, lds=ncols, ncols=ncols, ldn=1, Nt=Nt, S=S, Vd=V,
                 ldp=ncols)
        a.update(kw)
        return L.hyena_decode_sample_automaton(a["logits"], a["ldl"], a["dtype"], a["B"], a["V"], a["Vlive"], ctypes.c_float(a["T"]), a["top_k"],
                                               ctypes.c_float(a["top_p"]), a["seed"], a["eos"], a["pad"], a["col"], a["done"], a["seq"], a["lds"],
                                               a["ncols"], a["nxt"], a["ldn"], None, None, a["M"], a["Nt"], a["S"], a["delta"], a["Vd"],
                                               a["dstate"], a["start"], a["lp"], a["ldp"], None)

    def beam(**kw):
        a = dict(p, ldl=V, dtype=0, B=B, fan=fan, V=V, Vlive=12, eos=-1, pad=0, ldn=1, ncols=ncols, Nt=Nt, S=S, Vd=V, ldh=ncols, nrec=ncols)
        a.update(kw)
        return L.hyena_decode_beam_automaton(a["logits"], a["ldl"], a["dtype"], a["B"], a["fan"], a["V"], a["Vlive"], a["eos"], a["pad"], a["col"],
                                             a["done"], a["score"], a["start"], a["parent"], a["nxt"], a["ldn"], a["ncols"], a["M"], a["Nt"],
                                             a["S"], a["delta"], a["Vd"], a["dstate"], a["th"], a["ph"], a["lh"], a["ldh"], a["nrec"], None)

    tables = (dict(M=None), dict(delta=None), dict(dstate=None), dict(S=0), dict(S=4097), dict(Nt=0), dict(Nt=1025, S=4096), dict(Vd=V - 1),
              dict(Vd=V + 1), dict(V=12, Vlive=12, Vd=V))
    for name in ("logits", "seed", "col", "done", "seq", "nxt", "start"):
        assert sample(**{name: None}) == 1, name
    for kw in tables + (dict(V=65, ldl=65, Vd=65), dict(Vlive=0), dict(Vlive=17), dict(top_p=0.0), dict(top_p=1.5), dict(dtype=3), dict(ldl=V - 1),
                        dict(lds=ncols - 1), dict(ldp=0), dict(B=0)):
        assert sample(**kw) == 1, kw
    for name in ("logits", "col", "done", "score", "start", "parent", "nxt"):
        assert beam(**{name: None}) == 1, name
    for kw in tables + (dict(fan=0), dict(fan=17, B=34), dict(B=3), dict(V=65, ldl=65, Vd=65), dict(Vlive=0), dict(dtype=3), dict(ldl=V - 1),
                        dict(ncols=0), dict(ldn=0), dict(nrec=0), dict(ldh=ncols - 1)):
        assert beam(**kw) == 1, kw
    for k in ("seq", "col", "lp", "dstate", "th"):
        assert bool((t[k] == 0).all()), k                                       # nothing ran
    assert bool((t["parent"] == -5).all())
    if dev == "cpu":                                                            # (the emulation: the good calls really run)
        assert sample() == 0 and t["col"].tolist() == [1] * B and t["dstate"].tolist() == [1] * B
        assert beam() == 0 and t["col"].tolist() == [2] * B and beam(th=None, ph=None, lh=None) == 0 and sample(lp=None) == 0


# ---- 6. the language model -------------------------------------------------------------------------------------------------------------------------
B_LM, P_LM, N_LM, PAD = DC.B_LM, DC.P_LM, DC.N_LM, DC.PAD
LM_MODES = DC.LM_MODES
gen, new_tokens, mode_kwargs = DC.gen, DC.new_tokens, DC.mode_kwargs


def lm(dev):
    return DC.lm(dev)


def letters(toks):
    return "".join(LETTER.get(int(v), "x") for v in toks)


def prompt_rows(ids, lengths, fan=1):
    """the prompt of every returned row as a list of tokens"""
    rows = ids.cpu().tolist()
    if lengths is not None:
        rows = [r[:n] for r, n in zip(rows, lengths.cpu().tolist())]
    return [r for r in rows for _ in range(fan)]


def up_to_eos(toks, eos):
    toks = [int(v) for v in toks]
    return toks[:toks.index(eos)] if eos is not None and eos in toks else toks


def case_lm_fails_without_the_feature(dev, graphed):
    """the first three tokens the model writes greedily become the avoided motif: with the automaton no row writes them"""
    from hyena_dna_amd.inference import motif_automaton
    m = lm(dev)
    ids, _ = DS.lm_inputs(dev)
    free = new_tokens(gen(m, ids, allowed_tokens=ACGT), None)
    motif = letters(free[0, :3])
    assert "x" not in motif
    A = motif_automaton(avoid=[motif])
    for cg in (False, True)[:1 + graphed]:
        out = gen(m, ids, allowed_tokens=ACGT, automaton=A, cg=cg)
        toks = new_tokens(out, None)
        for b, prompt in enumerate(prompt_rows(ids, None)):
            text = letters(prompt[-2:]) + letters(toks[b])                       # an occurrence that ends in a new column
            assert motif not in text, (b, motif, text)
        assert not torch.equal(toks[0, :3], free[0, :3])


RESTRICTIVE = dict(avoid=["CG", "TA"], max_homopolymer=2, reverse_complement=True)


def implied_masks(A, M, prompts, toks, eos):
    """walk every returned row through the host automaton -> (B, N) int64: the mask M held at the row's state before each token"""
    B, N = toks.shape
    out = torch.full((B, N), -1, dtype=torch.int64)
    for b in range(B):
        s = A.initial_state(prompts[b])
        for i in range(N):
            out[b, i] = M[0 if M.shape[0] == 1 else i, s]
            t = int(toks[b, i])
            if t == eos:
                break
            assert (int(out[b, i]) >> t) & 1, (b, i, t)
            s = int(A.delta[s, t])
            assert s >= 0
    return out


def case_lm_replay_through_the_existing_kernel(dev, mode, graphed):
    """generate(automaton=A) and generate(constraints=the masks A implied along every row) are the same run, torch.equal"""
    from hyena_dna_amd.inference import automaton_step_tables, motif_automaton, token_mask
    m = lm(dev)
    ids, lengths, extra = mode_kwargs(mode, dev)
    fan = extra.get("num_return_sequences", 1)
    A = motif_automaton(**RESTRICTIVE)
    kw = dict(top_k=4, temperature=1.3, seed=17, vocab_size=12, output_logprobs=True, output_scores=True)
    for cg in (False, True)[:1 + graphed]:
        out = gen(m, ids, lengths, allowed_tokens=ACGT, automaton=A, cg=cg, **kw, **extra)
        toks = new_tokens(out, lengths, fan=fan)
        M = automaton_step_tables(A, N_LM, masks=torch.full((N_LM,), token_mask(ACGT)), vocab=12, positional=False)
        masks = implied_masks(A, M, prompt_rows(ids, lengths, fan), toks, None)
        assert bool((masks != token_mask(ACGT)).any())                          # the automaton does bite
        # (G, N) constraints cannot tell the rows of a group apart: one replay per member j of the groups, compared on its rows g fan + j
        # (the same layout, hence the same logits bit for bit; the draw depends on the row index, which the rows keep)
        for j in range(fan):
            again = gen(m, ids, lengths, constraints=masks[j::fan].contiguous().to(dev), cg=cg, **kw, **extra)
            assert torch.equal(again.sequences[j::fan], out.sequences[j::fan])
            assert torch.equal(again.logprobs[j::fan], out.logprobs[j::fan])
            assert torch.equal(torch.stack(again.scores)[:, j::fan], torch.stack(out.scores)[:, j::fan])
        for b, prompt in enumerate(prompt_rows(ids, lengths, fan)):
            assert A.accepts(toks[b].tolist(), A.initial_state(prompt))


def case_lm_membership(dev, graphed):
    from hyena_dna_amd.inference import motif_automaton
    m = lm(dev)
    ids, lengths = DS.lm_inputs(dev)
    eos = 11
    cases = [(dict(avoid=["GAT", "CC"], reverse_complement=True), None), (dict(max_homopolymer=2), None),
             (dict(require=["TATA"]), None), (dict(require=["TATA"], avoid=["AA"]), eos), (dict(require=["GCG", "CGC"], max_homopolymer=3), eos)]
    for kwA, e in cases:
        A = motif_automaton(**kwA)
        allowed = ACGT + ([e] if e is not None else [])
        for ln, cg, extra in ((None, False, {}), (lengths, False, {}), (None, True, dict(num_return_sequences=2)))[:2 + graphed]:
            fan = extra.get("num_return_sequences", 1)
            out = gen(m, ids, ln, allowed_tokens=allowed, automaton=A, eos_token_id=e, top_k=5, temperature=2.0, seed=3, vocab_size=12, cg=cg, **extra)
            toks = new_tokens(out, ln, fan=fan)
            for b, prompt in enumerate(prompt_rows(ids, ln, fan)):
                word = up_to_eos(toks[b], e)
                assert A.accepts(word, A.initial_state(prompt)), (kwA, e, b, letters(prompt), letters(word))
                if e is not None and len(word) < N_LM:
                    assert bool((toks[b, len(word) + 1:] == PAD).all())
                for motif in kwA.get("require", ()):                             # it occurs, and no row ends before it does
                    assert motif in letters(prompt[len(prompt) - A.context:]) + letters(word), (kwA, b, letters(word))
            if e is not None and not cg:                                         # stop_check_every reads `done` only: the same rows, fewer steps
                early = gen(m, ids, ln, allowed_tokens=allowed, automaton=A, eos_token_id=e, top_k=5, temperature=2.0, seed=3, vocab_size=12,
                            stop_check_every=1, **extra)
                assert torch.equal(early.sequences, out.sequences)
    # without the automaton the same calls do leave the language (the cases are not vacuous)
    A = motif_automaton(max_homopolymer=2)
    free = new_tokens(gen(m, ids, allowed_tokens=ACGT, top_k=5, temperature=2.0, seed=3, vocab_size=12), None)
    assert not all(A.accepts(free[b].tolist(), A.initial_state(p)) for b, p in enumerate(prompt_rows(ids, None)))


def case_lm_prompt_boundary(dev):
    import pytest
    from hyena_dna_amd.inference import TokenAutomaton, iupac_constraints, motif_automaton
    m = lm(dev)
    ids, _ = DS.lm_inputs(dev)
    ids = ids.clone()
    ids[:, -5:] = torch.tensor([TOK[c] for c in "GAATT"]).to(dev)
    A = motif_automaton(avoid=["GAATTC"])
    assert A.context == 5
    blind = TokenAutomaton(A.delta, A.accept, start=A.start, context=0)
    N = 6
    force_c = iupac_constraints("C" + "." * (N - 1)).to(dev)
    out = new_tokens(gen(m, ids, N=N, constraints=force_c, allowed_tokens=ACGT, automaton=blind), None, N=N)
    assert bool((out[:, 0] == TOK["C"]).all())                                  # context = 0: the site is completed across the boundary
    with pytest.raises(ValueError, match="row 0"):
        gen(m, ids, N=N, constraints=force_c, allowed_tokens=ACGT, automaton=A)
    out = new_tokens(gen(m, ids, N=N, constraints=iupac_constraints("M" + "." * (N - 1)).to(dev), allowed_tokens=ACGT, automaton=A), None, N=N)
    assert bool((out[:, 0] == TOK["A"]).all())
    for seed in range(8):
        out = new_tokens(gen(m, ids, N=N, allowed_tokens=ACGT, automaton=A, top_k=4, temperature=8.0, seed=seed), None, N=N)
        assert bool((out[:, 0] != TOK["C"]).all()), (seed, out[:, 0])
    firsts = torch.cat([new_tokens(gen(m, ids, N=N, allowed_tokens=ACGT, automaton=blind, top_k=4, temperature=8.0, seed=seed), None, N=N)[:, 0]
                        for seed in range(8)])
    assert bool((firsts == TOK["C"]).any())                                     # (the model does write C there when nothing holds it back)


def no_stop_codon_automaton(V=16):
    """by hand: the reading frame starts at the first new token; no in-frame TAA, TAG, TGA.  States: 0 codon start, 1 "T", 2 one base that
    is not T, 3 "TA", 4 "TG", 5 two bases that cannot become a stop"""
    a, c, g, t = ACGT
    delta = torch.zeros(6, V, dtype=torch.int32)
    delta[0], delta[0, t] = 2, 1
    delta[1], delta[1, a], delta[1, g] = 5, 3, 4
    delta[2] = 5
    delta[3], delta[3, a], delta[3, g] = 0, -1, -1
    delta[4], delta[4, a] = 0, -1
    delta[5] = 0
    from hyena_dna_amd.inference import TokenAutomaton
    return TokenAutomaton(delta)


def in_frame_stop(word):
    s = letters(word)
    return any(s[i:i + 3] in ("TAA", "TAG", "TGA") for i in range(0, len(s) - 2, 3))


def case_lm_raw_automaton_beams(dev, graphed):
    from hyena_dna_amd.inference import iupac_constraints
    A = no_stop_codon_automaton()
    G, P, N, k = 2, 8, 12, 4
    m = DB.lm(dev, 40)
    ids = DB.prompts(G, P, dev)
    free = DB.gen(m, ids, N, num_beams=k, num_return_sequences=k, constraints=iupac_constraints("TRN" * 4).to(dev))
    assert any(in_frame_stop(r) for r in free.sequences[:, P:].cpu().tolist())                 # unconstrained beams do hold stops
    for cg in (False, True)[:1 + graphed]:
        out = DB.gen(m, ids, N, num_beams=k, num_return_sequences=k, constraints=iupac_constraints("TRN" * 4).to(dev), automaton=A,
                     output_logprobs=True, cg=cg)
        words = out.sequences[:, P:].cpu().tolist()
        sc, lp = out.sequences_scores.cpu().double(), out.logprobs.cpu().double()
        fin = torch.isfinite(sc)
        assert bool(fin.view(G, k)[:, 0].all())
        for r, w in enumerate(words):
            if fin[r]:
                assert not in_frame_stop(w) and A.accepts(w), (r, letters(w))
        assert bool(((lp.sum(1) - sc).abs()[fin] <= (N * 1.01 * DB.E32 * lp.abs().sum(1))[fin]).all())
        assert bool((sc.view(G, k)[:, :-1] >= sc.view(G, k)[:, 1:]).all())
    # exhaustive: N = 3 and k = 16 keep every prefix.  T R N leaves 8 words, 5 of them accepted: exactly those come back, once each, ranked
    k, N = 16, 3
    out = DB.gen(m, ids, N, num_beams=k, num_return_sequences=k, constraints=iupac_constraints("TRN").to(dev), automaton=A)
    accepted = {tuple(TOK[c] for c in w) for w in ("TAC", "TAT", "TGC", "TGG", "TGT")}
    for g in range(G):
        sc = out.sequences_scores[g * k:(g + 1) * k].cpu()
        words = [tuple(w) for w in out.sequences[g * k:(g + 1) * k, P:].cpu().tolist()]
        n_fin = int(torch.isfinite(sc).sum())
        assert n_fin == len(accepted) and bool(torch.isfinite(sc[:n_fin]).all()) and bool((sc[:n_fin - 1] >= sc[1:n_fin]).all())
        assert set(words[:n_fin]) == accepted and len(set(words[:n_fin])) == n_fin, (g, words[:n_fin])
    # four free bases: 61 accepted words, the 16 best of them; every one accepted, none twice, ranked
    out = DB.gen(m, ids, N, num_beams=k, num_return_sequences=k, allowed_tokens=ACGT, automaton=A)
    for g in range(G):
        sc = out.sequences_scores[g * k:(g + 1) * k].cpu()
        words = [tuple(w) for w in out.sequences[g * k:(g + 1) * k, P:].cpu().tolist()]
        assert bool(torch.isfinite(sc).all()) and bool((sc[:-1] >= sc[1:]).all()) and len(set(words)) == k
        assert not any(in_frame_stop(w) for w in words)


def case_lm_graph_then_eager(dev):
    """GPU only: a generate call after a graphed one starts from the right state (the warm-up steps of the capture ran the real kernel and
    the snapshot put dstate back); cg = eager bit for bit is asserted inside the other cases"""
    from hyena_dna_amd.inference import motif_automaton
    m = lm(dev)
    ids, _ = DS.lm_inputs(dev)
    A = motif_automaton(**RESTRICTIVE)
    kw = dict(allowed_tokens=ACGT, automaton=A, top_k=4, temperature=1.3, seed=17, output_logprobs=True)
    eager = gen(m, ids, **kw)
    graphed = gen(m, ids, cg=True, **kw)
    after = gen(m, ids, **kw)
    again = gen(m, ids, cg=True, **kw)
    for o in (graphed, after, again):
        assert torch.equal(o.sequences, eager.sequences) and torch.equal(o.logprobs.view(torch.int32), eager.logprobs.view(torch.int32))
    b = dict(num_beams=4, num_return_sequences=4, allowed_tokens=ACGT, automaton=A, output_logprobs=True)
    eager, graphed = gen(m, ids, **b), gen(m, ids, cg=True, **b)
    assert torch.equal(eager.sequences, graphed.sequences) and torch.equal(eager.logprobs.view(torch.int32), graphed.logprobs.view(torch.int32))
    assert torch.equal(eager.sequences_scores.view(torch.int32), graphed.sequences_scores.view(torch.int32))
    for r, prompt in enumerate(prompt_rows(ids, None, 4)):
        assert A.accepts(eager.sequences[r, P_LM:].tolist(), A.initial_state(prompt))


def case_lm_refusals(dev):
    import pytest
    from hyena_dna_amd.inference import TokenAutomaton, iupac_constraints, motif_automaton
    m = lm(dev)
    ids, _ = DS.lm_inputs(dev)
    A = motif_automaton(avoid=["AA"])
    N = 4
    with pytest.raises(ValueError, match="sampler='device'"):
        gen(m, ids, N=N, automaton=A, sampler="torch")
    with pytest.raises(ValueError, match="use_cache=True"):
        m.generate(ids, max_length=P_LM + N, automaton=A)
    with pytest.raises(ValueError, match="out of scope"):
        gen(m, ids, N=N, automaton=A, constraints=torch.full((B_LM, N), -1, dtype=torch.int64).to(dev))
    with pytest.raises(ValueError, match="out of scope"):
        gen(m, ids, N=N, automaton=A, num_beams=2, constraints=torch.full((B_LM, N), -1, dtype=torch.int64).to(dev))
    with pytest.raises(ValueError, match="16 columns"):
        gen(m, ids, N=N, automaton=motif_automaton(avoid=["AA"], n_tokens=12))
    with pytest.raises(ValueError, match="TokenAutomaton"):
        gen(m, ids, N=N, automaton=A.delta)
    with pytest.raises(ValueError, match=r"row \d"):                            # avoid AA with positions forced to A, A
        gen(m, ids, N=N, automaton=A, constraints=iupac_constraints("AA..").to(dev))
    with pytest.raises(ValueError, match=r"row \d"):
        gen(m, ids, N=N, automaton=A, constraints=iupac_constraints("AA..").to(dev), num_beams=2)
    big = TokenAutomaton(torch.zeros(4096, 16, dtype=torch.int32), accept=torch.arange(4096) > 0)
    with pytest.raises(ValueError, match="2\\^22"):                             # before any cache: the length is never looked at
        gen(m, ids, N=1025, automaton=big)


def trivial_automaton(V=16):
    from hyena_dna_amd.inference import TokenAutomaton
    return TokenAutomaton(torch.zeros(1, V, dtype=torch.int32))


def case_lm_untouched_default(dev, mode):
    """without ``automaton`` generate runs what it ran before: all-ones constraints (the constrained kernel) against none (the plain one), as
    decode_constrain_local.case_lm_all_ones_is_todays_generate has it -- and the one-state automaton that allows everything is that run too"""
    m = lm(dev)
    if mode == "beam":
        ids, lengths, extra = DS.lm_inputs(dev)[0], None, dict(num_beams=3, num_return_sequences=3)
        kw = dict(output_logprobs=True)
    else:
        ids, lengths, extra = mode_kwargs(mode, dev)
        kw = dict(top_k=4, top_p=0.9, temperature=1.3, seed=11, output_scores=True, output_logprobs=True)
    ref = gen(m, ids, lengths, **kw, **extra)
    ones = gen(m, ids, lengths, constraints=torch.full((N_LM,), -1, dtype=torch.int64).to(dev), **kw, **extra)
    triv = gen(m, ids, lengths, automaton=trivial_automaton(), **kw, **extra)
    for out in (ones, triv):
        assert out._fields == ref._fields and torch.equal(out.sequences, ref.sequences)
        assert torch.equal(out.logprobs.view(torch.int32), ref.logprobs.view(torch.int32))
        if mode == "beam":
            assert torch.equal(out.sequences_scores.view(torch.int32), ref.sequences_scores.view(torch.int32))
        else:
            assert torch.equal(torch.stack(out.scores), torch.stack(ref.scores))
