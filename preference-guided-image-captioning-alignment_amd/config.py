"""YAML configuration with dotted access, the surface the reference's trainer and CLI read
(reference utils/config.py: ``Config(path)``, ``.get("a.b.c", default)``, ``.set``, ``get_stage{1,2}_config``,
``PGCA_*``-style environment overrides).  It parses the reference's ``configs/*.yaml`` unchanged and adds an
optional ``mi355x:`` section whose defaults reproduce the reference's behaviour.
"""
from __future__ import annotations

import os
from pathlib import Path
from typing import Any, Dict, Optional

import yaml

REQUIRED_SECTIONS = ("model", "training")

MI355X_DEFAULTS = {
    # reference_free True = the reference trainer's 2-forward loss; sft_alpha > 0 adds sft_alpha * NLL(chosen) to the loss
    "dpo": {"reference_free": True, "label_smoothing": 0.0, "sft_alpha": 0.0},
    # what Stage 2 trains on: "dpo" (as the reference), "caption" (the LM loss of steps.CaptionStep on the chosen captions)
    # or "caption_then_dpo" (caption phase, then DPO whose frozen reference policy is the captioner just trained), or
    # "mine_then_dpo" (DPO on pairs mined from the model's own captions: the "mining" section below);
    # caption_learning_rate: the caption phase's rate (null = training.stage2.learning_rate)
    "stage2": {"objective": "dpo", "caption_learning_rate": None},
    # mine_then_dpo: the keywords of mining.PreferenceMiner (num_candidates <= 64; rule adjacent | best_worst; threshold
    # is the reference's preference_threshold on the score difference; scorer alignment | logprob) and the seed of the
    # sampling generator (null = training.seed)
    "mining": {"num_candidates": 4, "rule": "adjacent", "threshold": 0.0, "scorer": "alignment", "max_length": 50,
               "min_tokens": 2, "temperature": 1.0, "top_p": 0.9, "top_k": 0, "repetition_penalty": 1.1,
               "no_repeat_ngram_size": 0, "decode_rows": 64, "seed": None},
    # caption metrics on the Stage-2 validation loader (evaluation.CaptionEvaluator) after every every_epochs-th epoch's
    # validation; 0 = never (the trainer then does, logs and returns what it did without this section); max_batches:
    # evaluate only the first so many batches (null = all)
    "evaluation": {"every_epochs": 0, "max_batches": None},
    "stage1": {"global_negatives": False},                      # False = local negatives, as the reference
    "allreduce_bucket_elems": 64 * 1024 * 1024,
    "allreduce_layer_group": 4,
    "clip_every_micro_step": False,                             # reference quirk
    "prefetch_depth": 2,                                        # batches prepared ahead on a side stream (0 = inline)
    "gpt2_pdrop": 0.1,                                          # HF GPT2Config embd/attn/resid dropout (train mode)
    "allreduce_bf16": False,                                    # bf16-compressed gradient all-reduce (halves xGMI bytes)
    "reset_best_val_between_stages": False,                     # False = as the reference: Stage 2 inherits best_val_loss
    "packed_rows": True,                                        # trunks run on the real tokens' rows only (same results)
}


RECOMPUTE_MODES = ("none", "mlp", "block")   # engine.GptTrunk.recompute


def select_recompute(config) -> str:
    """Activation-recompute mode of the GPT-2 trunks from a ``Config`` or a plain nested dict: ``mi355x.recompute``
    (``none | mlp | block``) when present, else the reference's ``hardware.gradient_checkpointing: true`` selects
    ``"block"`` (keep each layer's input, rebuild the rest in the backward - what ``gradient_checkpointing_enable()`` does
    per block), else ``"none"``.  ``mi355x.recompute`` has no entry in ``MI355X_DEFAULTS`` on purpose: an absent key must
    fall through to the reference's switch."""
    def get(path):
        cur = getattr(config, "config", config)
        for key in path.split("."):
            if not isinstance(cur, dict) or key not in cur:
                return None
            cur = cur[key]
        return cur

    mode = get("mi355x.recompute")
    if mode is None:
        return "block" if get("hardware.gradient_checkpointing") is True else "none"
    if mode is False:      # YAML reads a bare ``none``-like ``off`` / ``false`` as a boolean
        mode = "none"
    if mode not in RECOMPUTE_MODES:
        raise ValueError(f"mi355x.recompute must be one of {RECOMPUTE_MODES}, got {mode!r}")
    return mode


STAGE2_OBJECTIVES = ("dpo", "caption", "caption_then_dpo", "mine_then_dpo")


def select_objective(config) -> str:
    """``mi355x.stage2.objective`` of a ``Config`` or a plain nested dict (absent: ``"dpo"``, so the reference's configs
    select what they always did); anything but ``STAGE2_OBJECTIVES`` is a ``ValueError`` naming the key."""
    cur = getattr(config, "config", config)
    for key in ("mi355x", "stage2", "objective"):
        cur = cur.get(key) if isinstance(cur, dict) else None
    mode = MI355X_DEFAULTS["stage2"]["objective"] if cur is None else cur
    if mode not in STAGE2_OBJECTIVES:
        raise ValueError(f"mi355x.stage2.objective must be one of {STAGE2_OBJECTIVES}, got {mode!r}")
    return mode


def checkpoint_objective(ck: dict) -> str:
    """The Stage-2 objective a checkpoint dict was written under; one from before the key existed counts as ``"dpo"``."""
    return ck.get("mi355x_state", {}).get("objective", "dpo")


def select_evaluation(config) -> Optional[Dict[str, Any]]:
    """``mi355x.evaluation`` of a ``Config`` or a plain nested dict over its defaults, or ``None`` when
    ``every_epochs`` is 0 (the default): caption evaluation during training is off."""
    cur = getattr(config, "config", config)
    for key in ("mi355x", "evaluation"):
        cur = cur.get(key) if isinstance(cur, dict) else None
    unknown = sorted(set(cur or {}) - set(MI355X_DEFAULTS["evaluation"]))
    if unknown:
        raise ValueError(f"mi355x.evaluation: unknown keys {unknown}; known: {sorted(MI355X_DEFAULTS['evaluation'])}")
    section = {**MI355X_DEFAULTS["evaluation"], **(cur or {})}
    every = int(section["every_epochs"] or 0)
    if every < 0:
        raise ValueError(f"mi355x.evaluation.every_epochs must be >= 0, got {section['every_epochs']!r}")
    if every == 0:
        return None
    mb = section["max_batches"]
    return {"every_epochs": every, "max_batches": None if mb is None else int(mb)}


GENERATE_KEYS = {"max_length": int, "num_beams": int, "temperature": float, "do_sample": bool, "top_p": float,
                 "repetition_penalty": float, "length_penalty": float}


def generate_kwargs(config) -> Dict[str, Any]:
    """``evaluation.generate_config`` of a ``Config`` or a plain nested dict as keywords of ``CaptionDecoder.generate`` /
    ``generate_token_ids`` / ``generate_captions`` (the reference's evaluation script reads the same section key by
    key).  Keys the section does not set are left to ``generate``'s defaults; a missing section is a ``KeyError`` and
    a key ``generate`` does not know a ``ValueError``."""
    section = getattr(config, "config", config)["evaluation"]["generate_config"]
    unknown = sorted(set(section) - set(GENERATE_KEYS))
    if unknown:
        raise ValueError(f"evaluation.generate_config: unsupported keys {unknown}; known: {sorted(GENERATE_KEYS)}")
    return {k: GENERATE_KEYS[k](v) for k, v in section.items()}


class Config:
    def __init__(self, config_path: Optional[str] = None) -> None:
        if config_path is None:
            config_path = str(Path(__file__).resolve().parent.parent / "configs" / "default.yaml")
        self.config_path = Path(config_path)
        with open(self.config_path, "r", encoding="utf-8") as f:
            self.config: Dict[str, Any] = yaml.safe_load(f) or {}
        for sec in REQUIRED_SECTIONS:
            if sec not in self.config:
                raise ValueError(f"Missing required configuration section: {sec}")
        for st in ("stage1", "stage2"):
            if st not in self.config["training"]:
                raise ValueError(f"Missing required configuration section: training.{st}")
        self._apply_env_overrides()

    # the reference's own environment overrides (utils/config.py:91-136), same names, same targets
    REFERENCE_ENV = {
        "CONCEPTUAL_CAPTIONS_PATH": "data.conceptual_captions_path", "ULTRAFEEDBACK_PATH": "data.ultrafeedback_path",
        "CAPTION_ALIGNMENT_DATA_DIR": "data.conceptual_captions_path",
        "OUTPUT_DIR": "paths.output_dir", "CACHE_DIR": "paths.cache_dir",
        "CAPTION_ALIGNMENT_CACHE_DIR": "paths.cache_dir", "CAPTION_ALIGNMENT_OUTPUT_DIR": "paths.output_dir",
        "CAPTION_ALIGNMENT_LOG_DIR": "paths.log_dir",
        "CAPTION_ALIGNMENT_VISION_MODEL": "model.vision_model", "CAPTION_ALIGNMENT_TEXT_MODEL": "model.text_model",
        "CAPTION_ALIGNMENT_DEVICE": "hardware.device",
        "CAPTION_ALIGNMENT_BATCH_SIZE": "training.stage1.batch_size",
        "CAPTION_ALIGNMENT_LEARNING_RATE": "training.stage1.learning_rate",
        "CAPTION_ALIGNMENT_NUM_EPOCHS": "training.stage1.num_epochs", "CAPTION_ALIGNMENT_LOG_LEVEL": "logging.level",
        "WANDB_PROJECT": "logging.wandb_project", "WANDB_ENTITY": "logging.wandb_entity",
        "MLFLOW_EXPERIMENT": "logging.mlflow_experiment", "MLFLOW_TRACKING_URI": "logging.mlflow_tracking_uri",
        "CAPTION_ALIGNMENT_NUM_WORKERS": "data.num_workers", "CAPTION_ALIGNMENT_PIN_MEMORY": "data.pin_memory",
        "CAPTION_ALIGNMENT_MIXED_PRECISION": "hardware.mixed_precision",
        "CAPTION_ALIGNMENT_GRADIENT_CHECKPOINTING": "hardware.gradient_checkpointing",
    }

    @staticmethod
    def _convert_env_value(value: str) -> Any:
        """The reference's conversion (utils/config.py:151-182): booleans by name, then int, then float, else the string."""
        low = value.lower()
        if low in ("true", "1", "yes", "on"):
            return True
        if low in ("false", "0", "no", "off"):
            return False
        try:
            if "." not in value and "e" not in low:
                return int(value)
        except ValueError:
            pass
        try:
            return float(value)
        except ValueError:
            return value

    def _apply_env_overrides(self) -> None:
        """The reference's variables (``REFERENCE_ENV``: an empty value is ignored, as there), then this build's generic
        ``PGCA_CFG_<SECTION>__<KEY>[__<SUBKEY>]=value`` form (values parsed as YAML scalars)."""
        for name, path in self.REFERENCE_ENV.items():
            v = os.getenv(name)
            if v:
                self.set(path, self._convert_env_value(v))
        for k, v in os.environ.items():
            if not k.startswith("PGCA_CFG_"):
                continue
            path = k[len("PGCA_CFG_"):].lower().split("__")
            self.set(".".join(path), yaml.safe_load(v))

    def get(self, path: str, default: Any = None) -> Any:
        cur: Any = self.config
        try:
            for key in path.split("."):
                cur = cur[key]
            return cur
        except (KeyError, TypeError):
            if path.startswith("mi355x."):
                cur = MI355X_DEFAULTS
                try:
                    for key in path.split(".")[1:]:
                        cur = cur[key]
                    return cur
                except (KeyError, TypeError):
                    return default
            return default

    def set(self, path: str, value: Any) -> None:
        keys = path.split(".")
        cur = self.config
        for key in keys[:-1]:
            cur = cur.setdefault(key, {})
        cur[keys[-1]] = value

    def get_model_config(self) -> Dict[str, Any]:
        return self.config["model"]

    def get_training_config(self) -> Dict[str, Any]:
        return self.config["training"]

    def get_stage1_config(self) -> Dict[str, Any]:
        return self.config["training"]["stage1"]

    def get_stage2_config(self) -> Dict[str, Any]:
        return self.config["training"]["stage2"]

    def save(self, path: Optional[str] = None) -> None:
        with open(path or self.config_path, "w", encoding="utf-8") as f:
            yaml.safe_dump(self.config, f, default_flow_style=False, indent=2)

    def __repr__(self) -> str:
        return f"Config({self.config_path})"
