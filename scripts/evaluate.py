#!/usr/bin/env python3
"""Evaluate a checkpoint the trainer wrote: caption metrics over token ids (pgca_amd.evaluation) on the seeded synthetic
Stage-2 validation data scripts/train.py uses.

    python scripts/evaluate.py --config configs/default.yaml --checkpoint outputs/checkpoints/best_model_stage2.pt

Writes ``metrics.json`` and ``predictions.json`` (per image: the generated ids with the decoder's specials stripped,
their per-image CIDEr, and the text when the decoder's tokenizer is already on this machine - it is looked for with
``local_files_only=True`` and nothing is ever downloaded) into ``--output-dir``.
"""
import argparse
import json
import logging
import os
import sys

import torch
from torch.utils.data import DataLoader

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from pgca_amd.config import Config  # noqa: E402
from pgca_amd.evaluation import CaptionEvaluator  # noqa: E402
from train import SyntheticPairs, set_random_seeds, synthetic_image_size  # noqa: E402


def local_tokenizer(name: str):
    """The decoder's tokenizer if its files are on this machine, else None.  Never reaches for the network."""
    try:
        from transformers import AutoTokenizer
        return AutoTokenizer.from_pretrained(name, local_files_only=True)
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser(description="Caption metrics of a checkpoint (MI355X path)")
    ap.add_argument("--config", type=str, default=os.path.join(HERE, "..", "configs", "default.yaml"))
    ap.add_argument("--checkpoint", type=str, default=None, help="a checkpoint_*.pt / best_model_*.pt of the trainer; "
                    "without one the freshly initialised model is evaluated")
    ap.add_argument("--synthetic-samples", type=int, default=256)
    ap.add_argument("--output-dir", type=str, default="./evaluation_results")
    ap.add_argument("--batch-size", type=int, default=None, help="default: training.stage2.batch_size")
    args = ap.parse_args()
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(name)s %(levelname)s %(message)s")
    log = logging.getLogger("evaluate")
    cfg = Config(args.config)
    seed = int(cfg.get("training.seed", 42))
    set_random_seeds(seed)

    from pgca_amd.model import PreferenceGuidedCaptioningModel
    mc = cfg.get_model_config()
    model = PreferenceGuidedCaptioningModel(
        vision_model=mc.get("vision_model", "openai/clip-vit-base-patch32"),
        text_model=mc.get("text_model", "microsoft/DialoGPT-medium"), projection_dim=mc.get("projection_dim", 512),
        temperature=mc.get("temperature", 0.07), dropout=mc.get("dropout", 0.1),
        freeze_vision_backbone=mc.get("freeze_vision_backbone", False),
        freeze_text_backbone=mc.get("freeze_text_backbone", False), lora_config=mc.get("lora_config"), seed=seed)
    if args.checkpoint:
        ck = torch.load(args.checkpoint, map_location="cpu", weights_only=False)
        model.load_state_dict(ck["model_state_dict"], strict=True)
        model.sync_bf16()
        log.info(f"loaded {args.checkpoint} (stage {ck.get('stage')}, epoch {ck.get('epoch')})")

    bs = int(args.batch_size or cfg.get("training.stage2.batch_size", 8))
    S = int(cfg.get("data.max_caption_length", 128))
    side = synthetic_image_size(cfg.get("data.image_size", None), model.arch.vit.image, mc.get("vision_model"))
    vocab = model.arch.gpt.base_vocab
    # the Stage-2 validation set of scripts/train.py: same class, size rule and seed
    data = SyntheticPairs(max(bs, int(args.synthetic_samples * 0.1)), side, S, vocab, vocab, True, seed + 7 + 1)
    loader = DataLoader(data, batch_size=bs, shuffle=False, drop_last=False)

    evaluator = CaptionEvaluator(model, config=cfg)
    metrics = evaluator.evaluate(loader)
    os.makedirs(args.output_dir, exist_ok=True)
    with open(os.path.join(args.output_dir, "metrics.json"), "w", encoding="utf-8") as f:
        json.dump(metrics, f, indent=2, sort_keys=True)
    tok = local_tokenizer(mc.get("text_model", "microsoft/DialoGPT-medium"))
    last = evaluator.last
    predictions = []
    for i in range(metrics["num_samples"]):
        ids = last["pred_ids"][i, :int(last["length"][i])].tolist()
        row = {"index": i, "ids": ids, "cider": float(last["cider"][i]) * 10.0}
        if tok is not None:
            row["text"] = tok.decode(ids, skip_special_tokens=True).strip()
        predictions.append(row)
    with open(os.path.join(args.output_dir, "predictions.json"), "w", encoding="utf-8") as f:
        json.dump({"generate_config": evaluator.generate_kwargs, "text": tok is not None, "predictions": predictions}, f)
    log.info("metrics: " + " ".join(f"{k}={v:.6g}" if isinstance(v, float) else f"{k}={v}" for k, v in metrics.items()))
    log.info(f"wrote metrics.json and predictions.json to {args.output_dir}")


if __name__ == "__main__":
    main()
