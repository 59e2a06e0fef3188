"""The caption objective of Stage 2 through the trainer: ``mi355x.stage2.objective`` = ``caption`` and
``caption_then_dpo``, their checkpoints and the rule that a checkpoint resumes only a run of its own objective.
Synthetic loaders in the pattern of ``test_trainer_gpu.py`` / ``test_trainer_parity_gpu.py``."""
import math
import os

import numpy as np
import pytest
import torch

from pgca_amd import REPO_ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class ListLoader(list):
    """A loader is anything iterable with a length (the trainer only needs that)."""


def _pairs(arch, n, B, S, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        lens = torch.randint(4, S + 1, (2 * B,), generator=g)
        ids = torch.randint(0, arch.gpt.base_vocab, (2 * B, S), generator=g)
        mask = (torch.arange(S)[None] < lens[:, None]).long()
        out.append({"image": torch.randn(B, 3, arch.vit.image, arch.vit.image, generator=g),
                    "preferred_ids": ids[:B], "rejected_ids": ids[B:], "preferred_mask": mask[:B],
                    "rejected_mask": mask[B:]})
    return ListLoader(out)


def _config(out_dir, objective, epochs=2, dropout=0.0, **extra):
    from pgca_amd.config import Config
    cfg = Config(os.path.join(REPO_ROOT, "configs", "default.yaml"))
    cfg.set("paths.output_dir", str(out_dir))
    cfg.set("training.stage2.num_epochs", epochs)
    cfg.set("training.stage2.warmup_steps", 1)
    cfg.set("training.stage2.learning_rate", 1e-3)
    cfg.set("training.stage1.gradient_accumulation_steps", 2)   # one accumulation value governs both stages
    cfg.set("training.stage2.gradient_accumulation_steps", 2)
    cfg.set("training.stage2.logging_steps", 1)
    cfg.set("model.dropout", dropout)
    cfg.set("mi355x.gpt2_pdrop", dropout)
    if objective is not None:
        cfg.set("mi355x.stage2.objective", objective)
    for k, v in extra.items():
        cfg.set(k, v)
    return cfg


def _model(dropout=0.0, seed=21):
    from pgca_amd.arch import tiny_arch
    from pgca_amd.model import PreferenceGuidedCaptioningModel
    return PreferenceGuidedCaptioningModel(freeze_vision_backbone=True, arch=tiny_arch(), dropout=dropout, seed=seed,
                                           device=DEV)


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=False)


def test_caption_objective_trains_checkpoints_and_resumes(tmp_path):
    """Two epochs at accumulation 2 (train-mode dropout ON); then epoch 0's checkpoint loaded into a NEW model + trainer
    continues to the same result, under the criterion of test_resume_restores_optimizer_scheduler_and_continues."""
    from pgca_amd.trainer import PreferenceGuidedTrainer
    m1 = _model(0.1)
    train, val = _pairs(m1.arch, 4, 2, 16, seed=5), _pairs(m1.arch, 2, 2, 16, seed=6)
    d1 = tmp_path / "straight"
    t1 = PreferenceGuidedTrainer(m1, _config(d1, "caption", dropout=0.1), train, val, train, val)
    assert t1.objective == "caption" and t1.accum == 2
    before = m1.store.segments["decoder"].fp32.clone()
    o1 = t1.train_stage2()
    assert len(o1["train_loss"]) == 2 and all(np.isfinite(o1["train_loss"] + o1["val_loss"]))
    assert o1["train_loss"][1] < o1["train_loss"][0]                    # the same 4 batches twice: the LM loss must fall
    steps = [h["step_loss"] for h in t1.history if "step_loss" in h]
    assert len(steps) == 8 and all(math.isfinite(x) for x in steps)
    assert o1["train_loss"][0] > 0.5 * math.log(m1.arch.dec_vocab)      # an LM loss of an untrained decoder, not log 2
    assert not torch.equal(m1.store.segments["decoder"].fp32, before)
    ck0 = _load(d1 / "checkpoints" / "checkpoint_stage2_caption_epoch0.pt")
    assert ck0["stage"] == 2 and ck0["mi355x_state"]["objective"] == "caption" and ck0["mi355x_state"]["phase"] == "caption"
    assert (d1 / "checkpoints" / "best_model_stage2_caption.pt").exists()
    assert t1.reference_policy is None
    # resumed run
    m2 = _model(0.1)
    d2 = tmp_path / "resumed"
    t2 = PreferenceGuidedTrainer(m2, _config(d2, "caption", dropout=0.1), train, val, train, val)
    t2.load_checkpoint(str(d1 / "checkpoints" / "checkpoint_stage2_caption_epoch0.pt"))
    assert t2.best_val_loss == pytest.approx(o1["val_loss"][0])
    o2 = t2.train_stage2()
    assert len(o2["train_loss"]) == 1                                   # only epoch 1 ran
    assert o2["train_loss"][0] == pytest.approx(o1["train_loss"][1], abs=2e-6)
    assert o2["learning_rates"][0] == pytest.approx(o1["learning_rates"][1], rel=1e-6)
    for name in ("vision_head", "decoder"):
        a, b = m1.store.segments[name], m2.store.segments[name]
        np.testing.assert_allclose(b.fp32.cpu().numpy(), a.fp32.cpu().numpy(), rtol=0, atol=2e-6)
        np.testing.assert_allclose(b.exp_avg.cpu().numpy(), a.exp_avg.cpu().numpy(), rtol=0, atol=2e-6)
    ck1, ck2 = (_load(d / "checkpoints" / "checkpoint_stage2_caption_epoch1.pt") for d in (d1, d2))
    assert torch.equal(ck1["optimizer_state_dict"]["ctrl"][6:], ck2["optimizer_state_dict"]["ctrl"][6:])
    assert ck1["mi355x_state"]["dropout_step"] == ck2["mi355x_state"]["dropout_step"] == 8


def test_caption_then_dpo_snapshots_the_sft_model(tmp_path):
    from pgca_amd.trainer import PreferenceGuidedTrainer
    model = _model()
    train, val = _pairs(model.arch, 4, 2, 16, seed=7), _pairs(model.arch, 2, 2, 16, seed=8)
    cfg = _config(tmp_path, "caption_then_dpo", epochs=1, **{"mi355x.dpo.reference_free": False,
                                                             "mi355x.stage2.caption_learning_rate": 2e-3})
    initial = model.store.segments["decoder"].fp32.clone()
    tr = PreferenceGuidedTrainer(model, cfg, train, val, train, val)
    out = tr.train_stage2()
    assert len(out["train_loss"]) == 1 and len(out["caption_metrics"]["train_loss"]) == 1
    # the caption phase ran at its own rate, the DPO phase at Stage 2's
    assert out["caption_metrics"]["learning_rates"][0] != out["learning_rates"][0]
    sft = _load(tmp_path / "checkpoints" / "checkpoint_stage2_caption_epoch0.pt")
    assert sft["mi355x_state"]["objective"] == "caption_then_dpo" and sft["mi355x_state"]["phase"] == "caption"
    dpo = _load(tmp_path / "checkpoints" / "checkpoint_stage2_epoch0.pt")
    assert dpo["mi355x_state"]["phase"] == "dpo"
    # the frozen reference is the model the caption phase left: its weights, not the initial ones
    checked = 0
    for seg in tr.reference_policy.store.segments.values():
        for name in seg.index:
            assert torch.equal(seg.w(name).cpu(), sft["model_state_dict"][name]), name
            checked += 1
    assert checked > 20
    assert not torch.equal(tr.reference_policy.store.segments["decoder"].fp32, initial)
    assert not torch.equal(model.store.segments["decoder"].fp32, tr.reference_policy.store.segments["decoder"].fp32)
    # policy == reference when the DPO phase starts: its first micro-batch's loss is log 2
    first_dpo = [h["step_loss"] for h in tr.history if "step_loss" in h][len(train)]
    assert abs(first_dpo - math.log(2.0)) <= 1e-6
    # best_val_loss was reset between the phases: it is a DPO loss (about log 2), not the caption loss (several nats)
    assert tr.best_val_loss == pytest.approx(out["val_loss"][0]) and tr.best_val_loss < 1.0 < out["caption_metrics"]["val_loss"][0]


def test_a_caption_checkpoint_gives_a_dpo_run_its_weights_only(tmp_path):
    from pgca_amd.trainer import PreferenceGuidedTrainer
    m1 = _model()
    train, val = _pairs(m1.arch, 2, 2, 16, seed=9), _pairs(m1.arch, 2, 2, 16, seed=10)
    t1 = PreferenceGuidedTrainer(m1, _config(tmp_path / "a", "caption", epochs=1), train, val, train, val)
    t1.train_stage2()
    path = tmp_path / "a" / "checkpoints" / "checkpoint_stage2_caption_epoch0.pt"
    m2 = _model(seed=22)
    t2 = PreferenceGuidedTrainer(m2, _config(tmp_path / "b", None, epochs=1), train, val, train, val)
    assert t2.objective == "dpo"
    t2.load_checkpoint(str(path))
    assert torch.equal(m2.store.segments["decoder"].fp32, m1.store.segments["decoder"].fp32)     # the weights
    assert t2._resume is None and t2.epoch == 0 and t2.global_step == 0 and t2.best_val_loss == float("inf")
    out = t2.train_stage2()
    assert len(out["train_loss"]) == 1                                   # epoch 0 ran: nothing was skipped
    ck = _load(tmp_path / "b" / "checkpoints" / "checkpoint_stage2_epoch0.pt")
    assert float(ck["optimizer_state_dict"]["ctrl"][6]) == 1.0           # a fresh optimiser: its first step
    # ... while a checkpoint without the key is a dpo checkpoint and resumes a dpo run as before
    legacy = dict(ck, mi355x_state={k: v for k, v in ck["mi355x_state"].items() if k not in ("objective", "phase")})
    torch.save(legacy, tmp_path / "legacy.pt")
    t3 = PreferenceGuidedTrainer(_model(seed=23), _config(tmp_path / "c", None, epochs=1), train, val, train, val)
    t3.load_checkpoint(str(tmp_path / "legacy.pt"))
    assert t3._resume is not None and t3._resume["stage"] == 2 and t3.epoch == 0 and t3.global_step == ck["global_step"]
    # and a bad objective names its key
    with pytest.raises(ValueError, match="mi355x.stage2.objective"):
        PreferenceGuidedTrainer(_model(seed=24), _config(tmp_path / "d", "sft"), train, val, train, val)
