"""What beam search costs per token on the MI355X, next to the fan-out path it is built on.

    python scripts/bench_decode_beam.py [--prompts 1024,32768] [--beams 4,8] [--groups 1] [--tokens 256] [--repeats 7] [--out FILE]

Two calls at the same shape, END TO END (prefill, graph capture, every replay) over their new tokens, bf16 autocast, d_model 256 x 8 layers:
  beam     generate(num_beams=k, num_return_sequences=k, cg=True): per token the model step over the G k rows, the beam kernel and one
           re-parenting of every layer's cache, all in one replayed graph; one backtrack at the end
  fanout   generate(num_return_sequences=k, sampler="device", top_k=1, cg=True): the path of before over the same G k rows of the same fan-out
           cache, ending with the sampling kernel
so the difference is the beam kernel in the sampler's place plus the n_layer reorders.  After a warm-up of both, the two alternate
``--repeats`` times in one process; per variant the median and the run-to-run spread (max - min over the repeats) are reported.  Next to
the difference stands what the reorders of the LAST step move per layer, 2 B D N sizeof(bf16) bytes (N new tokens: the formula of
include/hyena_decode.h at its largest).  The JSON line is also written to ``--out`` (default profiles/decode_beam_bench.json)."""
import argparse
import json
import os
import statistics
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")          # before the HIP runtime starts (graphed steps)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D_MODEL, N_LAYER = 256, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompts", default="1024,32768")
    ap.add_argument("--beams", default="4,8")
    ap.add_argument("--groups", type=int, default=1)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_beam_bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)

    import torch
    from hyena_dna_amd.lm import HyenaDNALM

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    rows = []
    N, G = args.tokens, args.groups
    for P in [int(p) for p in args.prompts.split(",")]:
        L = P + N
        torch.manual_seed(0)
        layer = dict(l_max=L + 2, order=2, filter_order=64, emb_dim=5, short_filter_order=3, modulate=True, w=10, lr=6e-4, wd=0.0, lr_pos_emb=0.0)
        m = HyenaDNALM(d_model=D_MODEL, n_layer=N_LAYER, d_inner=4 * D_MODEL, vocab_size=12, layer=layer, resid_dropout=0.0, embed_dropout=0.1,
                       pad_vocab_size_multiple=8, fused_dropout_add_ln=True, residual_in_fp32=True).cuda().eval()
        ids = torch.randint(7, 11, (G, P), device="cuda")
        for k in [int(b) for b in args.beams.split(",")]:
            common = dict(max_length=L, use_cache=True, cg=True, vocab_size=12, return_dict_in_generate=True, num_return_sequences=k)
            calls = {"beam": lambda: m.generate(ids, num_beams=k, **common),
                     "fanout": lambda: m.generate(ids, sampler="device", top_k=1, **common)}
            ms = {v: [] for v in calls}
            with torch.autocast("cuda", dtype=torch.bfloat16):
                for fn in calls.values():                              # warm-up: tables, workspaces, GEMM heuristics, code objects
                    fn()
                for _ in range(args.repeats):
                    for v, fn in calls.items():
                        t, out = timed(fn)
                        assert out.sequences.shape == (G * k, L)
                        if v == "beam":
                            s = out.sequences_scores.view(G, k)
                            assert bool(torch.isfinite(s).all()) and bool((s[:, :-1] >= s[:, 1:]).all())
                        ms[v].append(t / N)
            row = {"prompt": P, "new_tokens": N, "prompts": G, "beams": k, "rows": G * k, "d_model": D_MODEL, "n_layer": N_LAYER, "repeats": args.repeats}
            for v, x in ms.items():
                row[f"{v}_ms_per_token"] = statistics.median(x)
                row[f"{v}_spread_ms"] = max(x) - min(x)
                row[f"{v}_all_ms"] = [round(t, 5) for t in x]
            row["beam_minus_fanout_ms"] = row["beam_ms_per_token"] - row["fanout_ms_per_token"]
            row["beyond_spreads"] = abs(row["beam_minus_fanout_ms"]) > max(row["beam_spread_ms"], row["fanout_spread_ms"])
            row["reorder_bytes_per_layer_last_step"] = 2 * G * k * D_MODEL * N * 2
            rows.append(row)
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
