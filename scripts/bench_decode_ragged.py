"""Per-token cost of the cached step with one position per row (``generate(lengths=...)``'s step) against the single-position step, with
HyenaDNALM in bf16 autocast (random init, eval mode).  Three variants at one shape, alternated ``--repeats`` times in one process:

    uniform         prefill without lengths: the single-position kernels (decode_pre / decode_conv / decode_post)
    rows_equal      prefill with lengths, all equal: the per-row kernels, one staged filter window per workgroup
    rows_distinct   prefill with lengths, all different: the per-row kernels restage the filter window for every row

    python scripts/bench_decode_ragged.py [--shape 32k] [--batch 8] [--tokens 64] [--repeats 3] [--out profiles/decode_ragged_bench.json]

Every time comes from device events around the steps after the prefill (eager, and replayed as one hipGraph).  Prints ONE JSON line and,
with ``--out``, writes it to that file."""
import argparse
import json
import os
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")          # before the HIP runtime starts (graphed steps)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from bench_decode import SHAPES, model, timed  # noqa: E402


def step_ms(m, ids, lengths, N, cg):
    """prefill (right-padded when lengths is given) + N - 1 steps; returns ms per step"""
    from hyena_dna_amd.inference import InferenceParams
    from hyena_dna_amd.lm import GraphedDecodeStep
    B, P = ids.shape
    ip = InferenceParams(max_seqlen=P + N, max_batch_size=B, lengths_per_sample=lengths)
    ip.key_value_memory_dict = m.allocate_inference_cache(B, P + N)
    logits = m(ids, inference_params=ip)[0].logits
    ip.seqlen_offset = P
    step = GraphedDecodeStep(m, ip, B) if cg else None
    nxt = logits[:, -1].argmax(-1, keepdim=True)
    steps = N - 1

    def loop():
        nonlocal nxt
        for _ in range(steps):
            out = step(nxt) if cg else m(nxt, inference_params=ip)[0].logits[:, -1]
            nxt = out.argmax(-1, keepdim=True)
            ip.seqlen_offset += 1
    ms, _ = timed(loop)
    if step is not None:
        step.release()
    del ip
    return ms / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="32k", choices=sorted(SHAPES))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import hyena_dna_amd  # noqa: F401
    from hyena_dna_amd import _lib
    _lib.lib()
    L, d, n_layer = SHAPES[args.shape]
    B, N = args.batch, args.tokens
    P = L - N
    m = model(L, d, n_layer)
    ids = torch.randint(7, 11, (B, P), device="cuda")
    equal = torch.full((B,), P, dtype=torch.int32, device="cuda")
    distinct = torch.tensor([P - 3 * j for j in range(B)], dtype=torch.int32, device="cuda")   # all different, every t mod 4, the same bytes as `equal`
    variants = {"uniform": None, "rows_equal": equal, "rows_distinct": distinct}
    row = {"shape": args.shape, "context": L, "d_model": d, "n_layer": n_layer, "B": B, "prompt": P, "new_tokens": N,
           "distinct_lengths": distinct.tolist(), "repeats": args.repeats}
    modes = [("eager", False)] + ([] if args.no_graph else [("graph", True)])
    times = {f"{v}_{mode}": [] for v in variants for mode, _ in modes}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        step_ms(m, ids[:, :min(P, 4096)], None, 4, False)                                                  # warm-up (tables, workspaces, GEMM heuristics)
        step_ms(m, ids, equal, 4, False)
        for _ in range(args.repeats):                                                                      # alternate the variants: same machine state for all
            for mode, cg in modes:
                for v, lengths in variants.items():
                    times[f"{v}_{mode}"].append(step_ms(m, ids, lengths, N, cg))
    for key, vals in times.items():
        row[key + "_ms_per_token"] = sorted(vals)[len(vals) // 2]
        row[key + "_ms_all"] = [round(x, 4) for x in vals]
    line = json.dumps({"metric": "decode_ragged_ms_per_token", "dtype": "bf16 autocast", "rows": [row]})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
