"""Cached generation with the lookahead carry against the plain cached step: ``generate(use_cache=True, cg=True, sampler="device", top_k=4,
lookahead=64)`` against ``lookahead=None`` (the parent commit's path, launch for launch), END TO END -- cache allocation, prefill, graph
capture and 256 new tokens -- with HyenaDNALM 256 x 8 layers in bf16 autocast (random init, eval mode).

    python scripts/bench_decode_lookahead.py [--shapes 1k:1,1k:8,32k:1,32k:8,1m:1,1m:8] [--new 256] [--W 64] [--repeats 7]
                                             [--out profiles/decode_lookahead_bench.json]

A shape is ``prompt:B``; the prompts are 1024, 32768 and 2^20 - 256 tokens.  After a warm-up of both, the two paths alternate ``--repeats``
times in one process with device events around each call; the median and the run-to-run spread (max - min) are reported, per call and per
new token, and ``faster_beyond_spread`` / ``slower_beyond_spread``: whether the medians differ by more than the two spreads combined.  The
same calls with ONE new token (prefill, allocation and the first draw; no step) are timed 3 times each, so that ``step_ms_per_token`` =
(median of N tokens - median of 1) / (N - 1) separates the steps from what both paths share.  The two paths' sequences are compared
(``tokens_equal_fraction``: sampling from logits that differ by rounding may part ways; each is held to the full forward in tests/).
``refresh_ms_per_layer`` / ``la_step_ms_per_layer`` / ``plain_step_ms_per_layer``: one layer's kernels alone on a prefilled cache -- one
refresh (hyena_decode_carry), one lookahead step (conv_la + post_la) and one plain step (decode_conv + decode_post), mean of 5 back-to-back
runs, median over the repeats.  Prints ONE JSON line and writes it to ``--out``."""
import argparse
import json
import os
import statistics
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")          # before the HIP runtime starts (graphed steps)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from bench_decode import model, timed  # noqa: E402

PROMPTS = {"1k": 1024, "32k": 32768, "1m": (1 << 20) - 256}
D_MODEL, N_LAYER = 256, 8


def stats(v):
    return {"median_ms": statistics.median(v), "spread_ms": max(v) - min(v), "all_ms": [round(x, 4) for x in v]}


def gen(m, ids, N, W):
    return timed(lambda: m.generate(ids, max_length=ids.shape[1] + N, use_cache=True, cg=N > 1, sampler="device", top_k=4, seed=0,
                                    lookahead=W))


def kernels_alone(m, ids, N, W, repeats, reps=5):
    from hyena_dna_amd import _lib
    from hyena_dna_amd.inference import InferenceParams
    B, P = ids.shape
    ip = InferenceParams(max_seqlen=P + N, max_batch_size=B, lookahead=W)
    ip.key_value_memory_dict = m.allocate_inference_cache(B, P + N, lookahead=W)
    m(ids, inference_params=ip)
    st = next(iter(ip.key_value_memory_dict.values()))
    plain_part = _lib.decode_partials(B, st.D, st.L, ids.device)

    def refresh():
        st.pos.fill_(P)
        return timed(lambda: [st.refresh() for _ in range(reps)])[0] / reps

    def la_step():                                        # the last position of the window: the most columns a step reads
        def one():
            st.pos.fill_(P + W - 1)
            _lib.decode_conv_la(st.k, st.hist, st.la_part, st.pos, st.base, B, W, st.L)
            _lib.decode_post_la(st.la_part, st.carry, st.hist, st.fb, st.x0, st.z, st.pos, st.base, B, st.L)
        return timed(lambda: [one() for _ in range(reps)])[0] / reps

    def plain_step():
        def one():
            st.pos.fill_(P + W - 1)
            _lib.decode_conv(st.k, st.hist, plain_part, st.pos, B, st.L)
            _lib.decode_post(plain_part, st.hist, st.fb, st.x0, st.z, st.pos, B, st.L)
        return timed(lambda: [one() for _ in range(reps)])[0] / reps

    refresh(), la_step(), plain_step()
    out = {"refresh_ms_per_layer": [], "la_step_ms_per_layer": [], "plain_step_ms_per_layer": []}
    for _ in range(repeats):
        out["refresh_ms_per_layer"].append(refresh())
        out["la_step_ms_per_layer"].append(la_step())
        out["plain_step_ms_per_layer"].append(plain_step())
    return {k: statistics.median(v) for k, v in out.items()}


def bench_shape(m, name, P, B, N, W, repeats):
    ids = torch.randint(7, 11, (B, P), device="cuda")
    a, b = gen(m, ids, N, W)[1], gen(m, ids, N, None)[1]                             # warm-up of both: code objects, allocator
    same = float((a[:, P:] == b[:, P:]).float().mean())
    del a, b
    gen(m, ids, 1, W), gen(m, ids, 1, None)
    res = {"lookahead": [], "plain": [], "lookahead_1": [], "plain_1": []}
    for i in range(repeats):
        res["lookahead"].append(gen(m, ids, N, W)[0])
        res["plain"].append(gen(m, ids, N, None)[0])
        if i < 3:
            res["lookahead_1"].append(gen(m, ids, 1, W)[0])
            res["plain_1"].append(gen(m, ids, 1, None)[0])
    la, pl = stats(res["lookahead"]), stats(res["plain"])
    la1, pl1 = statistics.median(res["lookahead_1"]), statistics.median(res["plain_1"])
    both = la["spread_ms"] + pl["spread_ms"]
    row = {"shape": name, "prompt": P, "B": B, "d_model": D_MODEL, "n_layer": N_LAYER, "new_tokens": N, "W": W, "repeats": repeats,
           "tokens_equal_fraction": same, "lookahead": la, "plain": pl,
           "lookahead_ms_per_token": la["median_ms"] / N, "plain_ms_per_token": pl["median_ms"] / N,
           "lookahead_spread_ms_per_token": la["spread_ms"] / N, "plain_spread_ms_per_token": pl["spread_ms"] / N,
           "lookahead_one_token_ms": la1, "plain_one_token_ms": pl1,
           "lookahead_step_ms_per_token": (la["median_ms"] - la1) / (N - 1), "plain_step_ms_per_token": (pl["median_ms"] - pl1) / (N - 1),
           "speedup_end_to_end": pl["median_ms"] / la["median_ms"],
           "faster_beyond_spread": bool(pl["median_ms"] - la["median_ms"] > both),
           "slower_beyond_spread": bool(la["median_ms"] - pl["median_ms"] > both)}
    torch.cuda.empty_cache()
    row.update(kernels_alone(m, ids, N, W, repeats))
    print(f"{name} B={B}: lookahead {la['median_ms']:.2f} ms (+-{la['spread_ms']:.2f}), plain {pl['median_ms']:.2f} ms (+-{pl['spread_ms']:.2f}) "
          f"for {N} tokens; steps {row['lookahead_step_ms_per_token']:.4f} vs {row['plain_step_ms_per_token']:.4f} ms per token; per layer "
          f"refresh {row['refresh_ms_per_layer']:.4f}, la step {row['la_step_ms_per_layer']:.4f}, plain step "
          f"{row['plain_step_ms_per_layer']:.4f} ms", file=sys.stderr, flush=True)
    return row


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1k:1,1k:8,32k:1,32k:8,1m:1,1m:8")
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--W", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "decode_lookahead_bench.json"))
    args = ap.parse_args()
    import hyena_dna_amd  # noqa: F401
    from hyena_dna_amd import _lib
    _lib.lib()
    rows, models = [], {}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for spec in [s for s in args.shapes.split(",") if s]:
            name, B = spec.split(":")
            P = PROMPTS[name]
            if name not in models:
                models.clear()
                torch.cuda.empty_cache()
                models[name] = model(P + args.new, D_MODEL, N_LAYER)
            rows.append(bench_shape(models[name], spec, P, int(B), args.new, args.W, args.repeats))
            torch.cuda.empty_cache()
    line = json.dumps({"metric": "generate_cg_device_sampler_lookahead_vs_plain_ms", "dtype": "bf16 autocast", "rows": rows})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
