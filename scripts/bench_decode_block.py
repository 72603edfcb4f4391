"""Appending T known tokens to a live decode cache: ONE block step (``HyenaDNALM.forward`` with (B, T) ids at ``seqlen_offset > 0`` and ``allow_append``:
decode_*_block, the history streamed once for the T positions) against T single-position steps on the same cache, both eager, with
HyenaDNALM in bf16 autocast (random init, eval mode).

    python scripts/bench_decode_block.py [--shapes 32k:1,32k:8,1m:1,1m:1x8] [--T 4,16,64] [--repeats 7] [--out profiles/decode_block_bench.json]

A shape is ``name:B`` (B independent sequences) or ``name:GxN`` (G prompts fanned out to N rows each: the ``fan=N`` cache layout).  Per
shape the cache is prefilled ONCE with a prompt of context - 64 tokens; before every measurement every layer's position and short-conv
tail are put back to where the prefill left them (the history columns the appended tokens write are overwritten by the next run: the
time does not depend on their values), so both paths append the same T tokens to the same cache.  After a warm-up of both, the two paths
alternate ``--repeats`` times in one process with device events around each; the median and the run-to-run spread (max - min) are
reported, and ``faster_beyond_spread``: whether the block step's median is below the single steps' by more than the two spreads
combined.  ``conv_*``: the long-convolution kernel of ONE layer alone on the same cache -- decode_conv_block once against decode_conv T
times (mean of 5 back-to-back runs, median over the repeats) -- with the bytes each streams and the ratio to the 1 / T the bytes promise.

The last row times ``score_continuations`` (n = 8 candidates of T = 64 tokens after one context of 2^20 - 64: one prefill + one block
forward) against 8 plain forwards over context + continuation.  Prints ONE JSON line and writes it to ``--out``."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from bench_decode import SHAPES, model, timed  # noqa: E402

TAIL = 64                                                # positions kept free behind the prompt: the longest block


def stats(v):
    return {"median_ms": statistics.median(v), "spread_ms": max(v) - min(v), "all_ms": [round(x, 5) for x in v]}


def conv_bytes(t0, T, D, G, n, S, calls, io_bytes=2):
    """what the long-convolution kernel streams per layer for T outputs in `calls` launches: filter window, shared history once per
    prompt, every row's own columns"""
    return calls * (D * (t0 + T) * 4 + G * D * S * io_bytes + G * n * D * (t0 + T - S) * io_bytes)


def bench_shape(m, name, L, G, n, Ts, repeats):
    from hyena_dna_amd import _lib
    from hyena_dna_amd.inference import InferenceParams
    B, P = G * n, L - TAIL
    d = m.lm_head.weight.shape[1]
    prompt = torch.randint(7, 11, (G, P), device="cuda")
    ip = InferenceParams(max_seqlen=L, max_batch_size=B, allow_append=True)
    ip.key_value_memory_dict = m.allocate_inference_cache(B, L, **(dict(fan=n, prompt_len=P) if n > 1 else {}))
    m(prompt, inference_params=ip)
    states = list(ip.key_value_memory_dict.values())
    tails = [st.tail.clone() for st in states]

    def rewind():
        for st, tl in zip(states, tails):
            st.pos.fill_(P)
            st.tail.copy_(tl)
        ip.seqlen_offset = P

    def block(ids):
        rewind()
        return timed(lambda: m(ids, inference_params=ip)[0].logits)

    def singles(ids):
        rewind()

        def loop():
            outs = []
            for i in range(ids.shape[1]):
                ip.seqlen_offset = P + i
                outs.append(m(ids[:, i:i + 1], inference_params=ip)[0].logits)
            return torch.cat(outs, dim=1)
        return timed(loop)

    st = states[0]

    def conv_only(T, blockwise, reps=5):
        rewind()
        if blockwise:
            part = st._block_buffers(B, T)[0]
            if n > 1:
                fn = lambda: _lib.decode_conv_block_fan(st.k, st.hist_shared, st.hist, part, st.pos, B, n, T, st.L, st.S)
            else:
                fn = lambda: _lib.decode_conv_block(st.k, st.hist, part, st.pos, B, T, st.L)
            calls = 1
        else:
            if n > 1:
                fn = lambda: _lib.decode_conv_fan(st.k, st.hist_shared, st.hist, st.part, st.pos, B, n, st.L, st.S)
            else:
                fn = lambda: _lib.decode_conv(st.k, st.hist, st.part, st.pos, B, st.L)
            calls = T                                     # (all at position P: the T positions differ by at most 63 of ~L columns)
        return timed(lambda: [fn() for _ in range(reps * calls)])[0] / reps

    rows = []
    for T in Ts:
        ids = torch.randint(7, 11, (B, T), device="cuda")
        zb, z1 = block(ids)[1], singles(ids)[1]                                   # warm-up: code objects, scratch
        close = ((zb.double() - z1.double()).norm() / z1.double().norm()).item()  # (the kernels agree bit for bit; the GEMMs see other shapes)
        conv_only(T, True), conv_only(T, False)
        res = {"block": [], "single_steps": [], "conv_block": [], "conv_single": []}
        for _ in range(repeats):
            res["block"].append(block(ids)[0])
            res["single_steps"].append(singles(ids)[0])
            res["conv_block"].append(conv_only(T, True))
            res["conv_single"].append(conv_only(T, False))
        blk, one = stats(res["block"]), stats(res["single_steps"])
        cb, c1 = statistics.median(res["conv_block"]), statistics.median(res["conv_single"])
        row = {"shape": name, "context": L, "d_model": d, "n_layer": len(states), "prompts": G, "fan": n, "B": B, "t0": P, "T": T, "repeats": repeats,
               "logits_rel_diff": close, "block": blk, "single_steps": one, "speedup": one["median_ms"] / blk["median_ms"],
               "faster_beyond_spread": bool(one["median_ms"] - blk["median_ms"] > one["spread_ms"] + blk["spread_ms"]),
               "conv_block_ms_per_layer": cb, "conv_single_steps_ms_per_layer": c1, "conv_ratio": cb / c1, "conv_ratio_by_bytes": 1.0 / T,
               "conv_block_bytes_per_layer": conv_bytes(P, T, d, G, n, st.S, 1), "conv_single_steps_bytes_per_layer": conv_bytes(P, 1, d, G, n, st.S, T)}
        row["conv_block_GBps"] = row["conv_block_bytes_per_layer"] / cb / 1e6
        row["conv_single_GBps"] = row["conv_single_steps_bytes_per_layer"] / c1 / 1e6
        print(f"{name} B={B} fan={n} T={T}: block {blk['median_ms']:.3f} ms (+-{blk['spread_ms']:.3f}), {T} steps {one['median_ms']:.3f} ms "
              f"(+-{one['spread_ms']:.3f}); conv per layer {cb:.4f} vs {c1:.4f} ms", file=sys.stderr, flush=True)
        rows.append(row)
    return rows


def bench_score(m, L, n, T, repeats):
    P = L - TAIL
    ctx = torch.randint(7, 11, (1, P), device="cuda")
    cont = torch.randint(7, 11, (1, n, T), device="cuda")
    full = torch.cat([ctx.expand(n, P), cont[0]], dim=1)

    def forwards():
        return [m(full[j:j + 1])[0].logits[:, P - 1:P + T - 1].float() for j in range(n)]
    a, b = timed(lambda: m.score_continuations(ctx, cont, vocab_size=12, return_logits=True))[1], timed(forwards)[1]      # warm-up
    ref = torch.cat(b)
    close = ((a[1][0].double() - ref.double()).norm() / ref.double().norm()).item()
    del a, b, ref
    res = {"score_continuations": [], "full_forwards": []}
    for _ in range(repeats):
        res["score_continuations"].append(timed(lambda: m.score_continuations(ctx, cont, vocab_size=12))[0])
        res["full_forwards"].append(timed(forwards)[0])
    s, f = stats(res["score_continuations"]), stats(res["full_forwards"])
    print(f"score_continuations n={n} T={T} P={P}: {s['median_ms']:.1f} ms vs {n} forwards {f['median_ms']:.1f} ms", file=sys.stderr, flush=True)
    return {"shape": "score_continuations", "context": P, "candidates": n, "T": T, "repeats": repeats, "logits_rel_diff": close,
            "score_continuations": s, "full_forwards": f, "speedup": f["median_ms"] / s["median_ms"],
            "faster_beyond_spread": bool(f["median_ms"] - s["median_ms"] > f["spread_ms"] + s["spread_ms"])}


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32k:1,32k:8,1m:1,1m:1x8")
    ap.add_argument("--T", default="4,16,64")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--score", default="1m", help="shape of the score_continuations row ('' to skip)")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "decode_block_bench.json"))
    args = ap.parse_args()
    import hyena_dna_amd  # noqa: F401
    from hyena_dna_amd import _lib
    _lib.lib()
    Ts = [int(t) for t in args.T.split(",")]
    rows, models = [], {}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for spec in [s for s in args.shapes.split(",") if s]:
            name, rows_spec = spec.split(":")
            G, n = (int(v) for v in rows_spec.split("x")) if "x" in rows_spec else (int(rows_spec), 1)
            L, d, n_layer = SHAPES[name]
            if name not in models:
                models.clear()
                torch.cuda.empty_cache()
                models[name] = model(L, d, n_layer)
            rows += bench_shape(models[name], spec, L, G, n, Ts, args.repeats)
            torch.cuda.empty_cache()
        if args.score:
            L, d, n_layer = SHAPES[args.score]
            if args.score not in models:
                models.clear()
                torch.cuda.empty_cache()
                models[args.score] = model(L, d, n_layer)
            rows.append(bench_score(models[args.score], L, 8, 64, args.repeats))
    line = json.dumps({"metric": "append_T_tokens_block_step_vs_T_single_steps_ms", "dtype": "bf16 autocast", "rows": rows})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
