"""Time one soft-prompt tuning step (forward, loss at the label positions, backward) on the reference's configuration
(configs/evals/soft_prompting_genomics.yaml on hyenadna-small-32k: d_model 256, 8 layers, bf16 autocast), B = 2, L = 32768, n soft tokens, four ways:

    fused / hidden_at      soft tokens inside the first norm, final norm + head on the label rows      (SoftPromptLM(fused=True).loss)
    unfused / hidden_at    torch.cat in front of the blocks, final norm + head on the label rows       (SoftPromptLM(fused=False).loss)
    fused / full           ... full-length logits, then the label rows                                 (what LitModel.step does after its forward)
    unfused / full

The variants are alternated in one process (one round = each variant once); the median of ``--rounds`` rounds and the spread (max - min) are
reported and written to ``--out``.

    python scripts/soft_prompt_bench.py --out profiles/soft_prompt_bench.json
"""
import argparse
import json
import os
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--soft-tokens", type=int, nargs="+", default=[2, 2048, 32768])
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--length", type=int, default=32768)
    ap.add_argument("--shots", type=int, default=5, help="label positions: 2 shots + 1, spread over the input")
    ap.add_argument("--d-model", type=int, default=256)
    ap.add_argument("--n-layer", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("soft_prompt_bench.py needs a ROCm device")
    from hyena_dna_amd.lm import HyenaDNALM, token_cross_entropy
    from hyena_dna_amd.soft_prompt import SoftPromptLM
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    B, L = args.batch, args.length
    layer = dict(l_max=L + max(args.soft_tokens) + 64, emb_dim=5, filter_order=64, short_filter_order=3, modulate=True, w=10, lr=6e-4, wd=0.0,
                 lr_pos_emb=0.0)
    lm = HyenaDNALM(d_model=args.d_model, n_layer=args.n_layer, d_inner=4 * args.d_model, vocab_size=12, layer=layer, resid_dropout=0.0,
                    embed_dropout=0.1, fused_dropout_add_ln=True, residual_in_fp32=True, pad_vocab_size_multiple=8).to(dev)
    ids = torch.randint(7, 11, (B, L), device=dev)
    n_pos = 2 * args.shots + 1
    pos = torch.linspace(L // n_pos, L - 1, n_pos, device=dev).long()
    results = []
    for n in args.soft_tokens:
        models = {f: SoftPromptLM(lm, n, soft_token_pdrop=0.1, fused=f).train() for f in (True, False)}

        def step(fused, at):
            m = models[fused]
            m.soft_tokens.grad = None
            with torch.autocast("cuda", dtype=torch.bfloat16):
                if at:
                    loss = m.loss(ids, pos)
                else:
                    loss = token_cross_entropy(m(ids)[:, pos - 1], ids[:, pos])
            loss.backward()
            return loss

        variants = [("fused/hidden_at", True, True), ("unfused/hidden_at", False, True), ("fused/full", True, False), ("unfused/full", False, False)]
        times = {v[0]: [] for v in variants}
        for r in range(args.warmup + args.rounds):
            for name, fused, at in variants:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0.record()
                step(fused, at)
                t1.record()
                torch.cuda.synchronize()
                if r >= args.warmup:
                    times[name].append(t0.elapsed_time(t1))
        for name, ts in times.items():
            ts = sorted(ts)
            rec = {"variant": name, "n_soft_tokens": n, "B": B, "L": L, "d_model": args.d_model, "n_layer": args.n_layer, "n_pos": n_pos,
                   "median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3), "spread_ms": round(ts[-1] - ts[0], 3),
                   "rounds": len(ts)}
            print(json.dumps(rec), flush=True)
            results.append(rec)
        del models
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "dtype": "bf16 autocast", "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
