"""What constraints and log-probs cost a user's call on the MI355X.

    python scripts/bench_decode_constrain.py [--shapes tiny,32k] [--batches 1,8] [--tokens 256] [--repeats 7] [--variants plain,constrained]
                                             [--package-root DIR] [--out FILE]

``generate(..., use_cache=True, cg=True, sampler="device", top_k=4, seed=0)`` END TO END (prefill, graph capture, every replay) over its new
tokens, bf16 autocast, once with no further argument (``plain``: hyena_decode_sample, the path of before) and once with
``allowed_tokens=[7, 8, 9, 10], output_logprobs=True`` (``constrained``: hyena_decode_sample_constrained as the graph's last node).  After a
warm-up of both, the variants alternate ``--repeats`` times in one process; per variant the median and the run-to-run spread (max - min over
the repeats) are reported, and the JSON line is also written to ``--out`` (default profiles/decode_constrain_bench.json).

``--package-root DIR --variants plain``: the same run with the package found under DIR (a checkout of another commit with its own library),
to show that the unconstrained path did not move."""
import argparse
import json
import os
import statistics
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")          # before the HIP runtime starts (graphed steps)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = {"tiny": (1024, 128, 2), "32k": (32768, 256, 8)}              # (context, d_model, n_layer)
VARIANTS = {"plain": {}, "constrained": dict(allowed_tokens=[7, 8, 9, 10], output_logprobs=True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="tiny,32k")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--variants", default="plain,constrained")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_constrain_bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))

    import torch
    import hyena_dna_amd
    from hyena_dna_amd.lm import HyenaDNALM
    assert os.path.abspath(hyena_dna_amd.__file__).startswith(os.path.abspath(args.package_root) + os.sep), hyena_dna_amd.__file__

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    rows = []
    for name in args.shapes.split(","):
        L, d, n_layer = SHAPES[name]
        torch.manual_seed(0)
        layer = dict(l_max=L + 2, order=2, filter_order=64, emb_dim=5, short_filter_order=3, modulate=True, w=10, lr=6e-4, wd=0.0, lr_pos_emb=0.0)
        m = HyenaDNALM(d_model=d, n_layer=n_layer, d_inner=4 * d, vocab_size=12, layer=layer, resid_dropout=0.0, embed_dropout=0.1,
                       pad_vocab_size_multiple=8, fused_dropout_add_ln=True, residual_in_fp32=True).cuda().eval()
        for B in [int(b) for b in args.batches.split(",")]:
            N = args.tokens
            P = L - N
            ids = torch.randint(7, 11, (B, P), device="cuda")
            calls = {v: (lambda v=v: m.generate(ids, max_length=L, use_cache=True, cg=True, sampler="device", top_k=4, seed=0,
                                                return_dict_in_generate=True, **VARIANTS[v])) for v in args.variants.split(",")}
            ms = {v: [] for v in calls}
            with torch.autocast("cuda", dtype=torch.bfloat16):
                for fn in calls.values():                              # warm-up: tables, workspaces, GEMM heuristics, code objects
                    fn()
                for _ in range(args.repeats):
                    for v, fn in calls.items():
                        t, out = timed(fn)
                        assert out.sequences.shape == (B, L)
                        if v == "constrained":
                            new = out.sequences[:, P:]
                            assert bool(((new >= 7) & (new <= 10)).all()) and out.logprobs.shape == (B, N) and bool(torch.isfinite(out.logprobs).all())
                        ms[v].append(t / N)
            row = {"shape": name, "context": L, "d_model": d, "n_layer": n_layer, "B": B, "prompt": P, "new_tokens": N, "repeats": args.repeats}
            for v, x in ms.items():
                row[f"{v}_ms_per_token"] = statistics.median(x)
                row[f"{v}_spread_ms"] = max(x) - min(x)
                row[f"{v}_all_ms"] = [round(t, 5) for t in x]
            if len(ms) == 2:
                row["constrained_minus_plain_ms"] = row["constrained_ms_per_token"] - row["plain_ms_per_token"]
                row["within_spread"] = row["constrained_minus_plain_ms"] <= max(row["plain_spread_ms"], row["constrained_spread_ms"])
            rows.append(row)
            torch.cuda.empty_cache()
        del m
        torch.cuda.empty_cache()
    line = json.dumps({"metric": "generate_cg_device_top_k4_end_to_end_ms_per_new_token", "dtype": "bf16 autocast", "rows": rows})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
