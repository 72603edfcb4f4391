"""Fine-tune a sequence classifier (hyena_dna_amd.classifier.HyenaDNAClassifier) on the synthetic planted-motif task of
``runner.make_synthetic_classification`` -- the stand-in for the GenomicBenchmarks sets, which need a download.

    python scripts/finetune_classify.py                      # 1500 steps at L <= 256, lr 6e-4: loss 0.69 -> 0.05, held-out accuracy 0.98 on one MI355X
    python scripts/finetune_classify.py --unfused            # the readout as final norm + reduction (comparison)
    python scripts/finetune_classify.py --pretrained lm.pt   # a HyenaDNALM state dict goes in through load_backbone

The model is the one ``experiment=hg38/genomic_benchmark`` describes (2 layers, d_model 128, pooled readout); batches are END-padded and the pad
positions are excluded from the pooled mean through the lengths the classifier counts on the device.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def build_classifier(d_model=128, n_layer=2, max_length=512, n_classes=2, mode="pool", fused_readout=True, embed_dropout=0.1, pad_token_id=4):
    from hyena_dna_amd.classifier import DNAEmbeddingModel, HyenaDNAClassifier, SequenceDecoder
    layer = dict(l_max=max_length + 2, emb_dim=5, filter_order=64, short_filter_order=3, modulate=True, w=10, lr=6e-4, wd=0.0, lr_pos_emb=0.0)
    backbone = DNAEmbeddingModel(d_model=d_model, n_layer=n_layer, d_inner=4 * d_model, vocab_size=12, layer=layer, resid_dropout=0.0,
                                 embed_dropout=embed_dropout, fused_dropout_add_ln=True, residual_in_fp32=True, pad_vocab_size_multiple=8)
    decoder = SequenceDecoder(backbone.d_output, d_output=n_classes, l_output=0, mode=mode)
    return HyenaDNAClassifier(backbone, decoder, pad_token_id=pad_token_id, fused_readout=fused_readout)


@torch.no_grad()
def evaluate(model, ids, labels, batch_size, dtype=torch.bfloat16):
    model.eval()
    hits = 0
    for i in range(0, ids.shape[0], batch_size):
        with torch.autocast(ids.device.type, dtype=dtype):
            logits = model(ids[i:i + batch_size])
        hits += (logits.argmax(-1) == labels[i:i + batch_size]).sum().item()
    model.train()
    return hits / ids.shape[0]


def finetune(model, train, heldout, steps, batch_size=32, lr=1e-3, weight_decay=0.1, dtype=torch.bfloat16, seed=0, log=None):
    """AdamW on mini-batches drawn with a fixed seed -> {"first_loss", "last_loss" (means of the first / last 10 steps), "accuracy" (held out),
    "majority" (the held-out majority-class rate)}"""
    ids, labels = train
    dev = ids.device
    opt = torch.optim.AdamW(model.parameters(), lr=lr, weight_decay=weight_decay)
    g = torch.Generator().manual_seed(seed)
    losses = []
    model.train()
    for step in range(steps):
        pick = torch.randint(0, ids.shape[0], (batch_size,), generator=g).to(dev)
        with torch.autocast(dev.type, dtype=dtype):
            loss = model.loss(ids[pick], labels[pick])
        opt.zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
        losses.append(loss.item())
        if log is not None and (step % 20 == 0 or step == steps - 1):
            log(f"step {step:5d}  loss {losses[-1]:.4f}")
    k = min(10, len(losses))
    h_ids, h_labels = heldout
    share = h_labels.float().mean().item()
    return {"first_loss": sum(losses[:k]) / k, "last_loss": sum(losses[-k:]) / k, "accuracy": evaluate(model, h_ids, h_labels, batch_size, dtype),
            "majority": max(share, 1.0 - share)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--max-length", type=int, default=256)
    ap.add_argument("--n-train", type=int, default=2048)
    ap.add_argument("--n-heldout", type=int, default=512)
    ap.add_argument("--lr", type=float, default=6e-4, help="(2e-3 did not leave loss = ln 2 at L <= 256)")
    ap.add_argument("--copies", type=int, default=1, help="how often the motif is planted in a positive sequence")
    ap.add_argument("--mode", default="pool", choices=["pool", "sum", "last", "first"])
    ap.add_argument("--unfused", action="store_true", help="final norm over all positions, then the reduction")
    ap.add_argument("--pretrained", default=None, help="a HyenaDNALM state dict (torch.save) to start the backbone from")
    ap.add_argument("--freeze-backbone", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("finetune_classify.py needs a ROCm device: the model's kernels have no CPU fallback")
    from hyena_dna_amd.classifier import load_backbone
    from hyena_dna_amd.runner import make_synthetic_classification
    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    model = build_classifier(max_length=args.max_length, mode=args.mode, fused_readout=not args.unfused)
    if args.pretrained:
        load_backbone(model, torch.load(args.pretrained, map_location="cpu"), freeze_backbone=args.freeze_backbone)
    model = model.to(dev)
    ids, _, labels = make_synthetic_classification(args.n_train, args.max_length, seed=args.seed, copies=args.copies)
    h_ids, _, h_labels = make_synthetic_classification(args.n_heldout, args.max_length, seed=args.seed + 1, copies=args.copies)
    out = finetune(model, (ids.to(dev), labels.to(dev)), (h_ids.to(dev), h_labels.to(dev)), args.steps, args.batch_size, lr=args.lr,
                   seed=args.seed, log=print)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
