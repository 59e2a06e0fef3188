#!/usr/bin/env python3
"""Time of the caption (SFT) step against the 2-forward DPO step it shares its kernels with.

Geometry C2 of ``bench.py``: ViT-B/32 (frozen) + GPT-2-M, S = 128, the synthetic length distribution of
``bench.synthetic_batch``, dropout 0.1, packed rows, AdamW + clip.  One process, one model, the two steps ALTERNATING
step by step, so both see the same clocks and the same neighbours:

* ``CaptionStep`` on 512 captions - the chosen and the rejected captions of 256 synthetic pairs, one image each;
* ``DPOStep(reference_free=True)`` on the same 256 pairs: the same 512 sequences and the same rows through the same
  decoder kernels (its ViT runs on 256 images, the caption step's on 512: the one difference in the launch lists
  besides the loss heads).

    python tools/caption_step_probe.py --out profiles/caption_step.json

``--only caption`` / ``--only dpo2`` runs the steps of one kind alone (no timing), for a kernel trace per kind.

Per step kind: ms per step as the MEDIAN of ``--steps`` (>= 20) steps timed one by one with device events after
``--warmup`` steps, min / max, and the DPO step's own spread, which is the margin the comparison is read against.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256, help="pairs of the DPO step; the caption step takes 2 x as many captions")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seq-len", type=int, default=128)
    ap.add_argument("--vision-model", default="openai/clip-vit-base-patch32")
    ap.add_argument("--text-model", default="gpt2-medium")
    ap.add_argument("--out", default=None, help="write the JSON here as well as to stdout")
    ap.add_argument("--only", choices=["caption", "dpo2"], default=None,
                    help="run the steps of one kind and nothing else, for a kernel trace of that kind alone "
                         "(rocprofv3 --kernel-trace --stats -- python tools/caption_step_probe.py --only caption)")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be >= 20: the reported figure is a median")

    import torch

    from bench import synthetic_batch
    from pgca_amd.arch import make_arch
    from pgca_amd.engine import DropoutPlan
    from pgca_amd.model import PreferenceGuidedCaptioningModel
    from pgca_amd.steps import CaptionStep, DPOStep, FusedOptimizer

    if not torch.cuda.is_available():
        raise SystemExit("caption_step_probe: no GPU - nothing here can be measured on the host")
    dev = torch.device("cuda", 0)
    arch = make_arch(args.vision_model, args.text_model, 512)
    model = PreferenceGuidedCaptioningModel(args.vision_model, args.text_model, 512, temperature=0.5,
                                            freeze_vision_backbone=True, device=dev, seed=42)
    parts = (model.store, model.ws, model.vision_encoder.tower, model.vision_encoder.head, model.caption_decoder.engine)
    steps = {"caption": CaptionStep(*parts, dropout=DropoutPlan(0.1, base_seed=42), packed=True),
             "dpo2": DPOStep(*parts, beta=0.1, reference_free=True, dropout=DropoutPlan(0.1, base_seed=42), packed=True)}
    segs = [model.store.segments["vision_head"], model.store.segments["decoder"]]
    opt = FusedOptimizer(segs, lr=1e-5, weight_decay=0.01, max_grad_norm=1.0, warmup_steps=500, total_steps=100000)
    nbatch = 4
    batches = {"caption": [], "dpo2": []}
    for i in range(nbatch):
        b = synthetic_batch(args.pairs, args.seq_len, arch.gpt.base_vocab, arch.gpt.base_vocab, seed=1234 + 1000 * i)
        batches["dpo2"].append(DPOStep.prepare(b, dev))
        batches["caption"].append(CaptionStep.prepare(
            {"image": torch.cat([b["image"], b["image"]]),
             "caption_ids": torch.cat([b["preferred_ids"], b["rejected_ids"]]),
             "caption_mask": torch.cat([b["preferred_mask"], b["rejected_mask"]])}, dev))
    rows = {k: sum(p["seq"].pack.Mp for p in v) / nbatch for k, v in batches.items()}
    scored = {k: sum(p["seq"].n_rows for p in v) / nbatch for k, v in batches.items()}
    assert rows["caption"] == rows["dpo2"] and scored["caption"] == scored["dpo2"]
    torch.cuda.synchronize()

    def one(kind, i):
        p = batches[kind][i % nbatch]
        opt.zero_grad()
        loss = steps[kind].loss_and_grads(p["image"], p["seq"])
        opt.step()
        return loss

    if args.only is not None:       # one kind alone, nothing compared: the process is being traced from outside
        for i in range(args.warmup + args.steps):
            one(args.only, i)
        torch.cuda.synchronize()
        print(json.dumps({"tool": "tools/caption_step_probe.py", "only": args.only, "steps_run": args.warmup + args.steps}))
        return 0

    times = {"caption": [], "dpo2": []}
    last = {}
    for i in range(args.warmup + args.steps):
        for kind in ("caption", "dpo2"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            last[kind] = one(kind, i)
            e1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                times[kind].append(e0.elapsed_time(e1))
    # the one launch-list difference besides the loss heads, timed alone: the ViT + head forward of the caption step's
    # images against the DPO step's (every image is encoded once, and the caption step brings one image per caption)
    vit_ms = {}
    for kind in ("caption", "dpo2"):
        t = []
        for i in range(args.warmup + args.steps):
            img = batches[kind][i % nbatch]["image"]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _, _, pooled = model.vision_encoder.tower.forward(img, False)
            model.vision_encoder.head.forward(pooled, img.shape[0], False)
            e1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                t.append(e0.elapsed_time(e1))
        vit_ms[kind] = statistics.median(t)

    out = {"tool": "tools/caption_step_probe.py",
           "workload": f"{args.vision_model} (frozen) + {args.text_model}, seq_len {args.seq_len}, dropout 0.1, packed rows, "
                       f"AdamW + clip; CaptionStep on {2 * args.pairs} captions vs DPOStep(reference_free=True) on "
                       f"{args.pairs} pairs (the same {2 * args.pairs} sequences)",
           "timing": f"median of {args.steps} single steps between device events after {args.warmup} warm-up steps; the "
                     "two steps alternate in one process",
           "packed_rows_per_step": rows["caption"], "scored_rows_per_step": scored["caption"], "steps": {}}
    for kind, t in times.items():
        out["steps"][kind] = {"ms_per_step_median": statistics.median(t), "ms_per_step_min": min(t),
                              "ms_per_step_max": max(t), "ms_per_step_stdev": statistics.pstdev(t),
                              "loss": float(last[kind]), "sequences_per_s": 2 * args.pairs / (statistics.median(t) * 1e-3)}
    c, d = out["steps"]["caption"], out["steps"]["dpo2"]
    out["caption_over_dpo2"] = c["ms_per_step_median"] / d["ms_per_step_median"]
    out["dpo2_spread_over_median"] = (d["ms_per_step_max"] - d["ms_per_step_min"]) / d["ms_per_step_median"]
    out["gap_ms"] = c["ms_per_step_median"] - d["ms_per_step_median"]
    out["inside_dpo2_spread"] = bool(d["ms_per_step_min"] <= c["ms_per_step_median"] <= d["ms_per_step_max"])
    out["vit_forward_ms_median"] = {"caption_images": vit_ms["caption"], "dpo2_images": vit_ms["dpo2"],
                                    "difference": vit_ms["caption"] - vit_ms["dpo2"]}
    out["gap_ms_without_the_extra_images"] = out["gap_ms"] - (vit_ms["caption"] - vit_ms["dpo2"])
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
