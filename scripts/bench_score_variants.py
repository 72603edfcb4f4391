#!/usr/bin/env python
"""Variant effect scoring on the MI355X: ``HyenaDNALM.score_variants`` (one reference pass + edited windows on device) against the two ways the
package offered before, alternated in one process under bf16 autocast at d_model 256 x 8 layers:

  (a) the M edited sequences through ``model(ids)``, in batches that fit (``--forward-batch``);
  (b) one ``score_continuations`` call per variant (context = the reference below the variant, one candidate of `horizon` tokens).

Per configuration (context L, M variants at random positions, horizon): median and spread (max - min) of ``--repeats`` runs of each way, the
reference pass and the window pass of ``forward_edited_windows`` timed separately, ``max_memory_allocated`` of a ``score_variants`` call, and the
largest difference of the llr between score_variants and way (a) on the variants both ran.  The baselines cost M forwards / M prefills: with
``--baseline-cap`` C they run on the first min(M, C) variants and the row says so (``baseline_variants``; ``*_per_variant_ms`` is what scales).

``--trace-only``: nothing but a few ``score_variants`` calls of the first configuration, for a kernel trace taken from outside
(``rocprofv3 --kernel-trace --stats -- python scripts/bench_score_variants.py --trace-only ...``): the two new kernels per launch.

One JSON line on stdout, also written to ``--out`` (default profiles/score_variants_bench.json)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from bench_decode import SHAPES, model, timed  # noqa: E402


def stats(v):
    return {"median_ms": statistics.median(v), "spread_ms": max(v) - min(v), "all_ms": [round(x, 4) for x in v]}


def variants(ref, M, seed):
    g = torch.Generator().manual_seed(seed)
    L = ref.shape[1]
    pos = torch.randint(1, L - 1, (M,), generator=g).cuda()
    alts = (ref[0, pos] - 7 + 1 + torch.randint(0, 3, (M,), generator=g).cuda()) % 4 + 7
    return pos, alts


def llr_from_forwards(m, ref, base_lsm, pos, alts, T, batch):
    """way (a): the edited sequences through model(ids), `batch` at a time; the same truncated llr"""
    L = ref.shape[1]
    out = []
    for i in range(0, pos.shape[0], batch):
        p, a = pos[i:i + batch], alts[i:i + batch]
        seqs = ref.expand(p.shape[0], L).clone()
        seqs[torch.arange(p.shape[0], device="cuda"), p] = a
        logits = m(seqs)[0].logits
        idx = p[:, None] + torch.arange(T + 1, device="cuda")[None, :]
        tok = ref[0][idx.clamp(max=L - 1)]
        rows = logits[torch.arange(p.shape[0], device="cuda")[:, None], idx[:, :T].clamp(max=L - 1)][..., :12].float()
        la = torch.log_softmax(rows, -1)
        lr = base_lsm[(idx - 1).clamp(max=L - 1)]
        site = (lr[:, 0].gather(-1, a[:, None]) - lr[:, 0].gather(-1, tok[:, :1])).squeeze(-1)
        nxt = tok[:, 1:, None]
        down = (la.gather(-1, nxt) - lr[:, 1:].gather(-1, nxt)).squeeze(-1).masked_fill(idx[:, 1:] > L - 1, 0)
        out.append(site + down.sum(-1))
    return torch.cat(out)


def by_continuations(m, ref, pos, alts, T):
    """way (b): one score_continuations call per variant (its own prefill of the variant's prefix)"""
    L = ref.shape[1]
    out = []
    for p, a in zip(pos.tolist(), alts.tolist()):
        n = min(T, L - p)
        cont = ref[:, p:p + n].clone()
        cont[0, 0] = a
        out.append(m.score_continuations(ref[:, :p], cont[:, None], vocab_size=12).sum())
    return out


def bench_config(m, name, L, M, T, repeats, cap, fwd_batch):
    ref = torch.randint(7, 11, (1, L), generator=torch.Generator().manual_seed(1)).cuda()
    pos, alts = variants(ref, M, seed=M + T)
    Mb = min(M, cap)
    idx = pos[:, None] + torch.arange(T, device="cuda")[None, :]
    window = ref[0][idx.clamp(max=L - 1)]
    window[:, 0] = alts
    from hyena_dna_amd.variants import EditWindowParams

    def phases():
        ew = EditWindowParams(pos, None, T)
        t_ref = timed(lambda: m(ref, inference_params=ew)[0].logits)[0]
        ew.phase = "window"
        return t_ref, timed(lambda: m(window, inference_params=ew)[0].logits)[0]
    base_lsm = torch.log_softmax(m(ref)[0].logits[0, :, :12].float(), -1)
    # warm-up of every shape the timed window uses, and the agreement of the two routes
    got = m.score_variants(ref, pos, alts, horizon=T, vocab_size=12).llr
    want = llr_from_forwards(m, ref, base_lsm, pos[:Mb], alts[:Mb], T, fwd_batch)
    by_continuations(m, ref, pos[:2], alts[:2], T)
    phases()
    diff = float((got[:Mb] - want).abs().max())
    torch.cuda.reset_peak_memory_stats()
    m.score_variants(ref, pos, alts, horizon=T, vocab_size=12)
    peak = torch.cuda.max_memory_allocated()
    res = {k: [] for k in ("score_variants", "reference_pass", "window_pass", "forwards", "continuations")}
    for _ in range(repeats):
        res["score_variants"].append(timed(lambda: m.score_variants(ref, pos, alts, horizon=T, vocab_size=12))[0])
        res["forwards"].append(timed(lambda: llr_from_forwards(m, ref, base_lsm, pos[:Mb], alts[:Mb], T, fwd_batch))[0])
        res["continuations"].append(timed(lambda: by_continuations(m, ref, pos[:Mb], alts[:Mb], T))[0])
        a, b = phases()
        res["reference_pass"].append(a)
        res["window_pass"].append(b)
    row = {"shape": name, "L": L, "M": M, "horizon": T, "repeats": repeats, "baseline_variants": Mb, "max_abs_llr_diff_vs_forwards": diff,
           "max_memory_allocated_bytes": peak}
    row.update({k: stats(v) for k, v in res.items()})
    row["forwards_per_variant_ms"] = row["forwards"]["median_ms"] / Mb
    row["continuations_per_variant_ms"] = row["continuations"]["median_ms"] / Mb
    if Mb == M:
        s, f = row["score_variants"], row["forwards"]
        row["faster_than_forwards_beyond_spread"] = bool(f["median_ms"] - s["median_ms"] > f["spread_ms"] + s["spread_ms"])
    print(f"{name} M={M} T={T}: score_variants {row['score_variants']['median_ms']:.1f} ms (+-{row['score_variants']['spread_ms']:.1f}) = reference "
          f"{row['reference_pass']['median_ms']:.1f} + windows {row['window_pass']['median_ms']:.1f}; {Mb} forwards "
          f"{row['forwards']['median_ms']:.1f} ms (+-{row['forwards']['spread_ms']:.1f}); {Mb} score_continuations "
          f"{row['continuations']['median_ms']:.1f} ms; llr diff {diff:.3g}; peak {peak / 2 ** 30:.2f} GiB", file=sys.stderr, flush=True)
    return row


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1m:64:64,1m:64:512,1m:1024:64,1m:1024:512,32k:64:64,32k:64:512,32k:1024:64,32k:1024:512",
                    help="shape:M:horizon, comma separated")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--baseline-cap", type=int, default=64, help="the baselines run on at most this many variants")
    ap.add_argument("--forward-batch", type=int, default=4, help="edited sequences per model(ids) call of way (a) (2^20: 1)")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "score_variants_bench.json"))
    args = ap.parse_args()
    import hyena_dna_amd  # noqa: F401
    from hyena_dna_amd import _lib
    _lib.lib()
    if not torch.cuda.is_available():
        raise SystemExit("bench_score_variants.py measures on the GPU: no device found")
    rows, models = [], {}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for spec in [s for s in args.configs.split(",") if s]:
            name, M, T = spec.split(":")
            L, d, n_layer = SHAPES[name]
            if name not in models:
                models.clear()
                torch.cuda.empty_cache()
                models[name] = model(L, d, n_layer)
            if args.trace_only:
                ref = torch.randint(7, 11, (1, L), generator=torch.Generator().manual_seed(1)).cuda()
                pos, alts = variants(ref, int(M), seed=int(M) + int(T))
                for _ in range(3):
                    models[name].score_variants(ref, pos, alts, horizon=int(T), vocab_size=12)
                torch.cuda.synchronize()
                return
            rows.append(bench_config(models[name], spec, L, int(M), int(T), args.repeats, args.baseline_cap,
                                     1 if L >= 1 << 19 else args.forward_batch))
            torch.cuda.empty_cache()
    line = json.dumps({"metric": "score_variants_vs_full_forwards_vs_score_continuations_ms", "dtype": "bf16 autocast", "rows": rows})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
