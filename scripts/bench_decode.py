"""Per-token cost of generation with HyenaDNALM (bf16 autocast, random init, eval mode): the recompute loop of ``generate()`` against the
cached step, eager (``use_cache=True``) and replayed as one hipGraph (``cg=True``), at the three shapes bench.py uses.  Prints ONE JSON line.

    python scripts/bench_decode.py [--shapes tiny,32k,1m] [--batches 1,8] [--tokens 64] [--no-recompute]
    python scripts/bench_decode.py --sampler [--shapes tiny,32k] [--batches 1,8] [--tokens 256] [--repeats 7] [--out FILE]

Every time comes from device events after a warm-up.  recompute: generate() over `--recompute-tokens` new tokens (each one a full forward over
the growing prefix), divided by their number.  cached: the steps after the prefill (the prefill itself is reported apart).  The decode
convolution's own time comes from a separate ``rocprofv3 --kernel-trace --stats`` run; its algorithmic bytes per layer and step are
D (t + 1) 4 + B D (t + 1) sizeof(io) (``conv_bytes_per_layer`` below).

``--sampler``: what a user's call costs -- ``generate(..., use_cache=True, cg=True, top_k=4)`` END TO END (prefill, graph capture, every step and
everything between the steps) over its new tokens, once with ``sampler="torch"`` (torch ops and a reallocated id tensor between the replays) and
once with ``sampler="device"`` (``seed=0``: the sampling kernel is the graph's last node).  After a warm-up of both, the two alternate
``--repeats`` times in one process; per sampler the median and the run-to-run spread (max - min over the repeats) are reported, and the JSON
line is also written to ``--out`` (default profiles/decode_sampler_bench.json)."""
import argparse
import json
import os
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")          # before the HIP runtime starts (graphed steps)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

SHAPES = {"tiny": (1024, 128, 2), "32k": (32768, 256, 8), "1m": (1 << 20, 256, 8)}       # (context, d_model, n_layer)


def model(L, d, n_layer):
    from hyena_dna_amd.lm import HyenaDNALM
    torch.manual_seed(0)
    layer = dict(l_max=L + 2, order=2, filter_order=64, emb_dim=5, short_filter_order=3, modulate=True, w=10, lr=6e-4, wd=0.0, lr_pos_emb=0.0)
    return HyenaDNALM(d_model=d, n_layer=n_layer, d_inner=4 * d, vocab_size=12, layer=layer, resid_dropout=0.0, embed_dropout=0.1,
                      pad_vocab_size_multiple=8, fused_dropout_add_ln=True, residual_in_fp32=True).cuda().eval()


def conv_bytes_per_layer(t, D, B, io_bytes=2):
    return D * (t + 1) * 4 + B * D * (t + 1) * io_bytes


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def cached_run(m, ids, N, cg):
    """prefill + N - 1 steps (the last of N sampled tokens needs no step); returns (prefill ms, ms per step)"""
    from hyena_dna_amd.inference import InferenceParams
    from hyena_dna_amd.lm import GraphedDecodeStep
    B, P = ids.shape
    ip = InferenceParams(max_seqlen=P + N, max_batch_size=B)
    ip.key_value_memory_dict = m.allocate_inference_cache(B, P + N)
    t_pre, logits = timed(lambda: m(ids, inference_params=ip)[0].logits[:, -1])
    ip.seqlen_offset = P
    step = GraphedDecodeStep(m, ip, B) if cg else None
    nxt = logits.argmax(-1, keepdim=True)
    steps = N - 1

    def loop():
        nonlocal nxt
        for _ in range(steps):
            out = step(nxt) if cg else m(nxt, inference_params=ip)[0].logits[:, -1]
            nxt = out.argmax(-1, keepdim=True)
            ip.seqlen_offset += 1
    t_steps, _ = timed(loop)
    if step is not None:
        step.release()
    del ip
    return t_pre, t_steps / steps


def sampler_rows(args):
    """generate(cg=True, top_k=4) end to end per new token, sampler="torch" against sampler="device", alternating"""
    import statistics
    rows = []
    for name in args.shapes.split(","):
        L, d, n_layer = SHAPES[name]
        m = model(L, d, n_layer)
        for B in [int(b) for b in args.batches.split(",")]:
            N = args.tokens
            P = L - N
            ids = torch.randint(7, 11, (B, P), device="cuda")
            calls = {s: (lambda s=s: m.generate(ids, max_length=L, use_cache=True, cg=True, top_k=4, sampler=s, **({"seed": 0} if s == "device" else {})))
                     for s in args.samplers.split(",")}
            ms = {s: [] for s in calls}
            with torch.autocast("cuda", dtype=torch.bfloat16):
                for fn in calls.values():                                                        # warm-up: tables, workspaces, GEMM heuristics, code objects
                    fn()
                for _ in range(args.repeats):
                    for s, fn in calls.items():
                        t, out = timed(fn)
                        assert out.shape == (B, L)
                        ms[s].append(t / N)
            row = {"shape": name, "context": L, "d_model": d, "n_layer": n_layer, "B": B, "prompt": P, "new_tokens": N, "repeats": args.repeats}
            for s, v in ms.items():
                row[f"{s}_ms_per_token"] = statistics.median(v)
                row[f"{s}_spread_ms"] = max(v) - min(v)
                row[f"{s}_all_ms"] = [round(x, 5) for x in v]
            rows.append(row)
            torch.cuda.empty_cache()
        del m
        torch.cuda.empty_cache()
    line = json.dumps({"metric": "generate_cg_top_k4_end_to_end_ms_per_new_token", "dtype": "bf16 autocast", "rows": rows})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sampler", action="store_true", help="time generate(cg=True, top_k=4) end to end, torch against device sampler")
    ap.add_argument("--samplers", default="torch,device")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "decode_sampler_bench.json"))
    ap.add_argument("--shapes", default=None, help="default: tiny,32k,1m (--sampler: tiny,32k)")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--tokens", type=int, default=None, help="default: 64 (--sampler: 256)")
    ap.add_argument("--recompute-tokens", type=int, default=0, help="0: 16 at contexts <= 32k, 4 beyond")
    ap.add_argument("--no-recompute", action="store_true")
    ap.add_argument("--no-graph", action="store_true")
    args = ap.parse_args()
    import hyena_dna_amd  # noqa: F401
    from hyena_dna_amd import _lib
    _lib.lib()
    args.shapes = args.shapes or ("tiny,32k" if args.sampler else "tiny,32k,1m")
    args.tokens = args.tokens or (256 if args.sampler else 64)
    if args.sampler:
        return sampler_rows(args)
    rows = []
    for name in args.shapes.split(","):
        L, d, n_layer = SHAPES[name]
        m = model(L, d, n_layer)
        for B in [int(b) for b in args.batches.split(",")]:
            N = args.tokens
            P = L - N
            row = {"shape": name, "context": L, "d_model": d, "n_layer": n_layer, "B": B, "prompt": P, "new_tokens": N}
            ids = torch.randint(7, 11, (B, P), device="cuda")
            try:
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                    cached_run(m, ids[:, :min(P, 4096)], 4, False)                               # warm-up (tables, workspaces, GEMM heuristics)
                    row["prefill_ms"], row["cached_eager_ms_per_token"] = cached_run(m, ids, N, False)
                    if not args.no_graph:
                        row["cached_graph_ms_per_token"] = cached_run(m, ids, N, True)[1]
                    if not args.no_recompute:
                        R = args.recompute_tokens or (16 if L <= 32768 else 4)
                        Pr = L - R
                        m.generate(ids[:, :Pr - 1], max_length=Pr + 1)                          # warm-up at this length
                        ms, _ = timed(lambda: m.generate(ids[:, :Pr], max_length=L))
                        row["recompute_ms_per_token"] = ms / R
                        row["recompute_tokens_timed"] = R
                        row["speedup_eager"] = row["recompute_ms_per_token"] / row["cached_eager_ms_per_token"]
                        if "cached_graph_ms_per_token" in row:
                            row["speedup_graph"] = row["recompute_ms_per_token"] / row["cached_graph_ms_per_token"]
                t = L - 1
                row["conv_bytes_per_step_all_layers"] = n_layer * conv_bytes_per_layer(t, d, B)
            except torch.cuda.OutOfMemoryError as e:
                row["skipped"] = f"out of memory: {str(e).splitlines()[0]}"
            rows.append(row)
            torch.cuda.empty_cache()
        del m
        torch.cuda.empty_cache()
    print(json.dumps({"metric": "decode_ms_per_token", "dtype": "bf16 autocast", "rows": rows}))


if __name__ == "__main__":
    main()
