"""``mi355x.evaluation`` in the trainer: a tiny Stage-2 DPO run of two epochs (tiny_arch, 8 training pairs, 4 validation
pairs, batch 4).  With ``every_epochs: 1`` the caption metrics of the validation loader follow every validation; with
the default the trainer returns exactly what it returned before the section existed."""
import math
import os

import pytest
import torch

from pgca_amd import REPO_ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class ListLoader(list):
    """A loader is anything iterable with a length (the trainer only needs that)."""


def _pairs(arch, batches, B, seed, S=10):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(batches):
        lens = torch.randint(3, S + 1, (2, B), generator=g)
        mask = (torch.arange(S)[None, None] < lens[..., None]).long()
        ids = torch.randint(0, arch.gpt.base_vocab, (2, B, S), generator=g)
        ids = torch.where(mask.bool(), ids, torch.full_like(ids, arch.gpt.base_vocab))
        out.append({"image": torch.randn(B, 3, arch.vit.image, arch.vit.image, generator=g),
                    "preferred_ids": ids[0], "preferred_mask": mask[0], "rejected_ids": ids[1], "rejected_mask": mask[1],
                    "preference_score": torch.ones(B)})
    return ListLoader(out)


def _config(out_dir, **extra):
    from pgca_amd.config import Config
    cfg = Config(os.path.join(REPO_ROOT, "configs", "default.yaml"))
    cfg.set("paths.output_dir", str(out_dir))
    for k, v in {"training.stage2.num_epochs": 2, "training.stage2.warmup_steps": 1, "training.stage2.batch_size": 4,
                 "training.stage2.learning_rate": 1e-3, "training.stage1.gradient_accumulation_steps": 1,
                 "training.stage2.gradient_accumulation_steps": 1, "training.stage2.logging_steps": 1,
                 "training.stage2.early_stopping_patience": 10, "model.dropout": 0.0, "mi355x.gpt2_pdrop": 0.0,
                 "evaluation.generate_config": {"max_length": 12, "num_beams": 1, "do_sample": False}, **extra}.items():
        cfg.set(k, v)
    return cfg


def _run(tmp_path, **extra):
    from pgca_amd.arch import tiny_arch
    from pgca_amd.model import PreferenceGuidedCaptioningModel
    from pgca_amd.trainer import PreferenceGuidedTrainer
    model = PreferenceGuidedCaptioningModel(freeze_vision_backbone=True, arch=tiny_arch(), dropout=0.0, seed=41, device=DEV)
    train, val = _pairs(model.arch, 2, 4, seed=1), _pairs(model.arch, 1, 4, seed=2)
    trainer = PreferenceGuidedTrainer(model, _config(tmp_path, **extra), None, None, train, val)
    return trainer, trainer.train_stage2()


def test_every_epoch_appends_finite_caption_metrics(tmp_path):
    trainer, out = _run(tmp_path, **{"mi355x.evaluation": {"every_epochs": 1}})
    assert set(out) == {"train_loss", "val_loss", "learning_rates", "eval"}
    assert len(out["val_loss"]) == 2 and len(out["eval"]) == 2
    for e in out["eval"]:
        assert e["num_samples"] == 4 and all(math.isfinite(float(v)) for v in e.values())
        assert {"bleu_1", "bleu_4", "cider", "diversity_1", "unique_caption_ratio", "preference_win_rate",
                "alignment_score", "latency_p95_ms", "mean_length"} <= set(e)
        assert 0.0 <= e["bleu_1"] <= 1.0 and 0.0 <= e["preference_win_rate"] <= 1.0 and e["mean_length"] <= 11
    logged = [h for h in trainer.history if h.get("eval") == "captions"]
    assert [h["epoch"] for h in logged] == [0, 1]
    assert len(trainer._eval_corpora) == 1                        # the references were read once, not once per epoch


def test_off_by_default_the_result_has_the_keys_it_had(tmp_path):
    trainer, out = _run(tmp_path)
    assert set(out) == {"train_loss", "val_loss", "learning_rates"} and len(out["val_loss"]) == 2
    assert trainer._eval_cfg is None and not trainer._eval_corpora
    assert not any("eval" in h for h in trainer.history)


def test_every_second_epoch_and_max_batches(tmp_path):
    trainer, out = _run(tmp_path, **{"mi355x.evaluation": {"every_epochs": 2, "max_batches": 1}})
    assert len(out["eval"]) == 1 and out["eval"][0]["num_samples"] == 4
    assert [h["epoch"] for h in trainer.history if h.get("eval") == "captions"] == [1]
