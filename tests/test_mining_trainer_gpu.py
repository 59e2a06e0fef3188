"""Stage 2 under ``mi355x.stage2.objective: mine_then_dpo``: the trainer mines its pairs from images alone (tiny_arch, 16
synthetic images, one epoch, batch 4) and then runs the ordinary DPO phase on them."""
import math
import os

import pytest
import torch

from pgca_amd import REPO_ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class ListLoader(list):
    """A loader is anything iterable with a length (the trainer only needs that)."""


def _images(arch, batches, B, seed, captions=False):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(batches):
        b = {"image": torch.randn(B, 3, arch.vit.image, arch.vit.image, generator=g)}
        if captions:        # a Stage-1 batch: the mining pass must not read these
            b["caption_ids"] = torch.randint(0, arch.gpt.base_vocab, (B, 8), generator=g)
            b["caption_mask"] = torch.ones(B, 8, dtype=torch.long)
        out.append(b)
    return ListLoader(out)


def _config(out_dir, **extra):
    from pgca_amd.config import Config
    cfg = Config(os.path.join(REPO_ROOT, "configs", "default.yaml"))
    cfg.set("paths.output_dir", str(out_dir))
    for k, v in {"training.stage2.num_epochs": 1, "training.stage2.warmup_steps": 1, "training.stage2.batch_size": 4,
                 "training.stage2.learning_rate": 1e-3, "training.stage1.gradient_accumulation_steps": 1,
                 "training.stage2.gradient_accumulation_steps": 1, "training.stage2.logging_steps": 1,
                 "model.dropout": 0.0, "mi355x.gpt2_pdrop": 0.0, "mi355x.stage2.objective": "mine_then_dpo",
                 "mi355x.dpo.reference_free": False,
                 "mi355x.mining": {"num_candidates": 4, "max_length": 12, "decode_rows": 32}, **extra}.items():
        cfg.set(k, v)
    return cfg


def _model(seed=21):
    from pgca_amd.arch import tiny_arch
    from pgca_amd.model import PreferenceGuidedCaptioningModel
    return PreferenceGuidedCaptioningModel(freeze_vision_backbone=True, arch=tiny_arch(), dropout=0.0, seed=seed, device=DEV)


def _check_trained(trainer, out, model, decoder_before, text_before):
    assert len(out["train_loss"]) == len(out["val_loss"]) == 1
    assert math.isfinite(out["train_loss"][0]) and math.isfinite(out["val_loss"][0])
    assert not torch.equal(model.store.segments["decoder"].fp32, decoder_before)
    assert torch.equal(model.store.segments["text_tower"].fp32, text_before)          # the scorer is only read
    logged = [h for h in trainer.history if "mined_pairs" in h]
    assert [h["mined"] for h in logged] == ["train", "validation"]
    assert logged[0]["mined_images"] == 16 and logged[0]["mined_pairs"] >= 4
    assert 0.0 < logged[0]["pairs_per_image"] <= 3.0 and 0.0 <= logged[0]["candidates_left_out"] < 1.0
    steps = [h["step_loss"] for h in trainer.history if "step_loss" in h]
    assert len(steps) == logged[0]["mined_pairs"] // 4 and all(math.isfinite(x) for x in steps)
    # the frozen reference is the policy itself when the DPO phase starts: log 2 whatever the pairs are
    assert abs(steps[0] - math.log(2.0)) <= 1e-6 and trainer.reference_policy is not None


def test_an_image_only_stage2_loader_trains(tmp_path):
    from pgca_amd.trainer import PreferenceGuidedTrainer
    model = _model()
    train, val = _images(model.arch, 4, 4, seed=5), _images(model.arch, 1, 4, seed=6)
    trainer = PreferenceGuidedTrainer(model, _config(tmp_path), None, None, train, val)
    assert trainer.objective == "mine_then_dpo"
    before = model.store.segments["decoder"].fp32.clone(), model.store.segments["text_tower"].fp32.clone()
    out = trainer.train_stage2()
    _check_trained(trainer, out, model, *before)
    ck = torch.load(tmp_path / "checkpoints" / "checkpoint_stage2_epoch0.pt", map_location="cpu", weights_only=False)
    assert ck["mi355x_state"]["objective"] == "mine_then_dpo" and ck["mi355x_state"]["phase"] == "dpo"


def test_without_a_stage2_loader_the_stage1_images_are_mined(tmp_path):
    from pgca_amd.trainer import PreferenceGuidedTrainer
    model = _model(seed=22)
    train, val = _images(model.arch, 4, 4, seed=7, captions=True), _images(model.arch, 1, 4, seed=8, captions=True)
    trainer = PreferenceGuidedTrainer(model, _config(tmp_path), train, val, None, None)
    before = model.store.segments["decoder"].fp32.clone(), model.store.segments["text_tower"].fp32.clone()
    out = trainer.train_stage2()
    _check_trained(trainer, out, model, *before)


def test_an_impossible_threshold_names_its_key(tmp_path):
    """No cosine margin reaches 10: zero pairs, and the error says which key to lower."""
    from pgca_amd.trainer import PreferenceGuidedTrainer
    model = _model(seed=23)
    train = _images(model.arch, 1, 4, seed=9)
    cfg = _config(tmp_path, **{"mi355x.mining": {"num_candidates": 4, "max_length": 12, "threshold": 10.0}})
    with pytest.raises(RuntimeError, match=r"mi355x\.mining\.threshold"):
        PreferenceGuidedTrainer(model, cfg, None, None, train, None).train_stage2()
