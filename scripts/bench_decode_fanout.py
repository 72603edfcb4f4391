"""n continuations of one prompt: ``generate(num_return_sequences=n)`` (one prefill, the history below the prompt's last whole 8192-position
chunk kept once per prompt: decode_*_fan) against today's way, the prompt replicated n times (``generate(prompt.repeat(n, 1))``), with
HyenaDNALM in bf16 autocast (random init, eval mode).

    python scripts/bench_decode_fanout.py [--shapes 32k,1m] [--fan 8] [--tokens 64] [--repeats 7] [--out profiles/decode_fanout_bench.json]

Both paths run what ``generate(use_cache=True, cg=True, sampler="device", top_k=4, seed=0)`` runs -- the cache, the prefill, the sampler kernel
as the last node of one captured hipGraph, one replay per token -- with device events around the prefill and around the replays, so that
the per-token time is the step's and the prefill is reported apart.  After a warm-up of both, the two paths alternate ``--repeats`` times in
one process; per path the median and the run-to-run spread (max - min over the repeats) of the per-token time, the median prefill time
and ``torch.cuda.max_memory_allocated`` of one run are reported.  Prints ONE JSON line and writes it to ``--out``."""
import argparse
import json
import os
import statistics
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")          # before the HIP runtime starts (graphed steps)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from bench_decode import SHAPES, model, timed  # noqa: E402


def conv_bytes_per_layer(t, D, G, n, S, io_bytes=2):
    """what decode_conv streams per layer and step: the filter, the shared history once per prompt, every row's own columns"""
    return D * (t + 1) * 4 + G * D * S * io_bytes + G * n * D * (t + 1 - S) * io_bytes


def run(m, prompt, n, N, fan):
    """the prompt continued n times over N new tokens; fan: one prefill and the shared history, else the replicated prompt.
    Returns (prefill ms, ms per token over the N - 1 replays, peak bytes, sequences)."""
    from hyena_dna_amd.inference import DeviceSampler, InferenceParams
    from hyena_dna_amd.lm import GraphedDecodeStep
    dev = prompt.device
    G, P = prompt.shape
    B = G * n
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ids = prompt if fan else prompt.repeat_interleave(n, 0)
    seq = torch.zeros(B, P + N, dtype=torch.int64, device=dev)
    seq[:, :P] = prompt.repeat_interleave(n, 0)
    col = torch.full((B,), P, dtype=torch.int32, device=dev)
    ip = InferenceParams(max_seqlen=P + N, max_batch_size=B)
    ip.key_value_memory_dict = m.allocate_inference_cache(B, P + N, **(dict(fan=n, prompt_len=P) if fan else {}))
    t_pre, last = timed(lambda: m(ids, inference_params=ip)[0].logits[:, -1])
    if fan:
        last = last.repeat_interleave(n, 0)
    smp = DeviceSampler(seq, col, torch.zeros(1, dtype=torch.int64, device=dev), top_k=4, V=last.shape[-1])
    ip.seqlen_offset = P
    step = GraphedDecodeStep(m, ip, B, sampler=smp)
    smp(last, step.ids)

    def loop():
        for _ in range(N - 1):
            step.replay()
            ip.seqlen_offset += 1
    t_steps, _ = timed(loop)
    step.release()
    peak = torch.cuda.max_memory_allocated()
    del ip, smp, step
    return t_pre, t_steps / (N - 1), peak, seq


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32k,1m")
    ap.add_argument("--fan", type=int, default=8)
    ap.add_argument("--prompts", type=int, default=1)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "decode_fanout_bench.json"))
    args = ap.parse_args()
    import hyena_dna_amd  # noqa: F401
    from hyena_dna_amd import _lib
    _lib.lib()
    rows = []
    n, G, N = args.fan, args.prompts, args.tokens
    for name in args.shapes.split(","):
        L, d, n_layer = SHAPES[name]
        m = model(L, d, n_layer)
        P = L - N
        prompt = torch.randint(7, 11, (G, P), device="cuda")
        paths = {"fanout": True, "replicated": False}
        res = {p: [] for p in paths}
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            seqs = {p: run(m, prompt, n, N, fan)[3] for p, fan in paths.items()}                   # warm-up: tables, workspaces, code objects
            same = bool(torch.equal(seqs["fanout"], seqs["replicated"]))                          # the same tokens either way (same seed, same rows)
            del seqs
            for _ in range(args.repeats):
                for p, fan in paths.items():
                    torch.cuda.empty_cache()
                    res[p].append(run(m, prompt, n, N, fan)[:3])
                    print(f"{name} {p}: prefill {res[p][-1][0]:.1f} ms, {res[p][-1][1]:.4f} ms per token", file=sys.stderr, flush=True)
        S = P // _lib.DECODE_CHUNK * _lib.DECODE_CHUNK
        row = {"shape": name, "context": L, "d_model": d, "n_layer": n_layer, "prompts": G, "fan": n, "B": G * n, "prompt": P, "shared_columns": S,
               "new_tokens": N, "repeats": args.repeats, "sequences_equal": same,
               "conv_bytes_per_step_all_layers": {"fanout": n_layer * conv_bytes_per_layer(L - 1, d, G, n, S),
                                                  "replicated": n_layer * conv_bytes_per_layer(L - 1, d, G, n, 0)}}
        for p, v in res.items():
            tok = [x[1] for x in v]
            row[f"{p}_ms_per_token"] = statistics.median(tok)
            row[f"{p}_spread_ms"] = max(tok) - min(tok)
            row[f"{p}_all_ms"] = [round(x, 5) for x in tok]
            row[f"{p}_prefill_ms"] = statistics.median(x[0] for x in v)
            row[f"{p}_max_memory_allocated"] = max(x[2] for x in v)
        rows.append(row)
        del m
        torch.cuda.empty_cache()
    line = json.dumps({"metric": "generate_cg_device_top_k4_fanout_vs_replicated_ms_per_token", "dtype": "bf16 autocast", "rows": rows})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
