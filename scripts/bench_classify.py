"""Time the pooled readout of a sequence classifier -- fused (block.dropout_add_layer_norm_pool: one pass over hidden + residual) against the
unfused route on the same tree (dropout_add_layer_norm over all positions, then an fp32 reduction) -- forward + backward, and one training
step of a classifier either way.  Warm-up, then the median of repeated runs timed with device events; the two routes alternate.

    python scripts/bench_classify.py --out profiles/classify_bench.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def _time(fns, warmup, reps):
    """{name: [ms, ...]} -- the functions take turns, one timed call each per repetition"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return times


def _summary(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "runs": len(ts)}


def readout(B, L, D, warmup, reps):
    from hyena_dna_amd.block import dropout_add_layer_norm, dropout_add_layer_norm_pool, masked_pool
    dev = torch.device("cuda", 0)
    x0 = torch.randn(B, L, D, device=dev).to(torch.bfloat16).requires_grad_(True)
    res = torch.randn(B, L, D, device=dev).requires_grad_(True)
    w = torch.ones(D, device=dev, requires_grad=True)
    b = torch.zeros(D, device=dev, requires_grad=True)
    gp = torch.randn(B, D, device=dev)

    def fused():
        y = dropout_add_layer_norm_pool(x0, res, w, b, 0.0, 1e-5)
        torch.autograd.grad(y, [x0, res, w, b], gp)

    def unfused():
        y = masked_pool(dropout_add_layer_norm(x0, res, w, b, 0.0, 1e-5, prenorm=False, residual_in_fp32=True), None, "mean")
        torch.autograd.grad(y, [x0, res, w, b], gp)

    t = _time({"fused": fused, "unfused": unfused}, warmup, reps)
    io = B * L * D
    return {"shape": [B, L, D], "dtype": "bf16", "what": "readout forward + backward (final add + LayerNorm + mean over positions)",
            "fused": _summary(t["fused"]), "unfused": _summary(t["unfused"]),
            # bytes the fused pass has to move: forward reads x0 (2) + residual (4); backward reads them again and writes dx0 (2) + d_residual (4)
            "fused_min_bytes": io * (6 + 12)}


def train_step(B, L, D, n_layer, warmup, reps):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import finetune_classify as ft
    dev = torch.device("cuda", 0)
    out = {"shape": [B, L, D], "n_layer": n_layer, "dtype": "bf16 autocast", "what": "classifier training step (forward, loss, backward, AdamW), eager"}
    ids = torch.randint(7, 11, (B, L), device=dev)
    labels = torch.randint(0, 2, (B,), device=dev)
    models, fns = {}, {}
    for name, fused in (("fused", True), ("unfused", False)):
        torch.manual_seed(0)
        m = ft.build_classifier(d_model=D, n_layer=n_layer, max_length=L, fused_readout=fused, pad_token_id=None).to(dev)
        opt = torch.optim.AdamW(m.parameters(), lr=1e-4)
        models[name] = (m, opt)

        def step(m=m, opt=opt):
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = m.loss(ids, labels)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        fns[name] = step
    t = _time(fns, warmup, reps)
    out["fused"], out["unfused"] = _summary(t["fused"]), _summary(t["unfused"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_classify.py measures on a ROCm device; there is nothing to time without one")
    doc = {"command": "python scripts/bench_classify.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0),
           "timing": f"device events, {args.warmup} warm-up calls, median of {args.reps} runs, routes alternating", "results": []}
    for B, L in ((1, 1 << 20), (8, 32768)):
        doc["results"].append(readout(B, L, 256, args.warmup, args.reps))
        print(json.dumps(doc["results"][-1]), flush=True)
    for B, L, D, nl in ((8, 32768, 256, 2), (1, 1 << 20, 256, 2), (32, 1024, 128, 2)):
        doc["results"].append(train_step(B, L, D, nl, max(2, args.warmup // 2), max(5, args.reps // 3)))
        print(json.dumps(doc["results"][-1]), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
