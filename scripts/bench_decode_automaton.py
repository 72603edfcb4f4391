"""What an automaton costs a user's call on the MI355X.

    python scripts/bench_decode_automaton.py [--prompts 1024,32768] [--batches 1,8] [--tokens 256] [--repeats 7] [--modes sample,beam]
                                             [--out FILE]
    python scripts/bench_decode_automaton.py --trace            # a short workload for a kernel trace run of its own

``generate(..., use_cache=True, cg=True, sampler="device", top_k=4, seed=0, allowed_tokens=ACGT, output_logprobs=True)`` END TO END
(prefill, graph capture, every replay) over 256 new tokens at d_model 256 x 8 layers, bf16 autocast -- once as it is (``plain``:
hyena_decode_sample_constrained, the path of before) and once with ``automaton=motif_automaton(avoid=["GAATTC", "GGTCTC"],
reverse_complement=True, max_homopolymer=5)`` (``automaton``: hyena_decode_sample_automaton as the graph's last node; the tables are built
inside the call, so their cost is in the figure).  ``beam``: the same pair for ``num_beams=4`` (hyena_decode_beam against
hyena_decode_beam_automaton).  After a warm-up of both, the two alternate ``--repeats`` times in one process; per variant the median and
the run-to-run spread (max - min over the repeats) are reported, and whether the difference exceeds the larger of the two spreads.  The
JSON line is also written to ``--out`` (default profiles/decode_automaton_bench.json)."""
import argparse
import json
import os
import statistics
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")          # before the HIP runtime starts (graphed steps)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D_MODEL, N_LAYER = 256, 8
ACGT = [7, 8, 9, 10]
MODES = {"sample": dict(sampler="device", top_k=4, seed=0, allowed_tokens=ACGT, output_logprobs=True),
         "beam": dict(num_beams=4, allowed_tokens=ACGT, output_logprobs=True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompts", default="1024,32768")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--modes", default="sample,beam")
    ap.add_argument("--trace", action="store_true", help="a few eager calls of every variant at the shortest prompt, B = 1, and nothing else")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_automaton_bench.json"))
    args = ap.parse_args()

    import torch
    from hyena_dna_amd.inference import motif_automaton
    from hyena_dna_amd.lm import HyenaDNALM

    A = motif_automaton(avoid=["GAATTC", "GGTCTC"], reverse_complement=True, max_homopolymer=5)
    avoided = [[ACGT["ACGT".index(c)] for c in s] for s in ("GAATTC", "GGTCTC", "GAGACC")]
    N = args.tokens

    def model(P):
        torch.manual_seed(0)
        layer = dict(l_max=P + N + 2, order=2, filter_order=64, emb_dim=5, short_filter_order=3, modulate=True, w=10, lr=6e-4, wd=0.0, lr_pos_emb=0.0)
        return HyenaDNALM(d_model=D_MODEL, n_layer=N_LAYER, d_inner=4 * D_MODEL, vocab_size=12, layer=layer, resid_dropout=0.0, embed_dropout=0.1,
                          pad_vocab_size_multiple=8, fused_dropout_add_ln=True, residual_in_fp32=True).cuda().eval()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    def check(out, P, constrained):
        new = out.sequences[:, P:]
        assert bool(((new >= 7) & (new <= 10)).all()) and bool(torch.isfinite(out.logprobs).all())
        if constrained:
            for site in avoided:
                w = new.unfold(1, len(site), 1)
                assert not bool((w == torch.tensor(site, device=w.device)).all(-1).any()), site
            assert not bool((new.unfold(1, 6, 1) == new.unfold(1, 6, 1)[..., :1]).all(-1).any())       # no run of six

    if args.trace:
        P = min(int(p) for p in args.prompts.split(","))
        m = model(P)
        ids = torch.randint(7, 11, (1, P), device="cuda")
        with torch.autocast("cuda", dtype=torch.bfloat16):
            for mode in args.modes.split(","):
                for extra in ({}, dict(automaton=A)):
                    for _ in range(2):
                        m.generate(ids, max_length=P + 64, use_cache=True, return_dict_in_generate=True, **MODES[mode], **extra)
        torch.cuda.synchronize()
        return

    rows = []
    for P in [int(p) for p in args.prompts.split(",")]:
        m = model(P)
        for B in [int(b) for b in args.batches.split(",")]:
            ids = torch.randint(7, 11, (B, P), device="cuda")
            for mode in args.modes.split(","):
                calls = {v: (lambda extra=extra: m.generate(ids, max_length=P + N, use_cache=True, cg=True, return_dict_in_generate=True,
                                                             **MODES[mode], **extra))
                         for v, extra in (("plain", {}), ("automaton", dict(automaton=A)))}
                ms = {v: [] for v in calls}
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    for fn in calls.values():                          # warm-up: tables, workspaces, GEMM heuristics, code objects
                        fn()
                    for _ in range(args.repeats):
                        for v, fn in calls.items():
                            t, out = timed(fn)
                            check(out, P, v == "automaton")
                            ms[v].append(t / N)
                row = {"mode": mode, "d_model": D_MODEL, "n_layer": N_LAYER, "B": B, "prompt": P, "new_tokens": N, "repeats": args.repeats,
                       "automaton_states": A.S}
                for v, x in ms.items():
                    row[f"{v}_ms_per_token"] = statistics.median(x)
                    row[f"{v}_spread_ms"] = max(x) - min(x)
                    row[f"{v}_all_ms"] = [round(t, 5) for t in x]
                row["automaton_minus_plain_ms"] = row["automaton_ms_per_token"] - row["plain_ms_per_token"]
                row["exceeds_spread"] = abs(row["automaton_minus_plain_ms"]) > max(row["plain_spread_ms"], row["automaton_spread_ms"])
                rows.append(row)
                print(json.dumps(row), flush=True)
                torch.cuda.empty_cache()
        del m
        torch.cuda.empty_cache()
    line = json.dumps({"metric": "generate_cg_end_to_end_ms_per_new_token", "dtype": "bf16 autocast", "rows": rows})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
