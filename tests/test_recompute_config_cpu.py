"""Which activation-recompute mode the trainer asks of the GPT-2 trunks (``config.select_recompute``): the reference's
``hardware.gradient_checkpointing`` is honoured, ``mi355x.recompute`` overrides it, and a config with neither key (this
project's own ``configs/default.yaml``) keeps every activation as before."""
import copy
import os

import pytest
import yaml

from pgca_amd.config import Config, select_recompute

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the sections of the reference's configs/default.yaml that matter here, as its YAML parses
REFERENCE_STYLE = {
    "model": {"vision_model": "openai/clip-vit-base-patch32", "text_model": "microsoft/DialoGPT-medium", "dropout": 0.1},
    "training": {"seed": 42, "stage1": {"batch_size": 32, "num_epochs": 5}, "stage2": {"batch_size": 16, "num_epochs": 3}},
    "hardware": {"device": "auto", "mixed_precision": True, "gradient_checkpointing": True, "compile_model": False},
}


def _cfg(**sections):
    c = copy.deepcopy(REFERENCE_STYLE)
    for k, v in sections.items():
        c[k] = v
    return c


def test_reference_gradient_checkpointing_selects_block():
    assert select_recompute(REFERENCE_STYLE) == "block"


def test_mi355x_key_overrides_the_reference_key():
    for mode in ("none", "mlp", "block"):
        assert select_recompute(_cfg(mi355x={"recompute": mode})) == mode
    hw_off = dict(REFERENCE_STYLE["hardware"], gradient_checkpointing=False)
    assert select_recompute(_cfg(hardware=hw_off, mi355x={"recompute": "mlp"})) == "mlp"


def test_neither_key_keeps_everything():
    c = _cfg()
    del c["hardware"]["gradient_checkpointing"]
    assert select_recompute(c) == "none"
    del c["hardware"]
    assert select_recompute(c) == "none"
    assert select_recompute(_cfg(hardware={"gradient_checkpointing": False})) == "none"
    assert select_recompute(_cfg(mi355x={"packed_rows": True})) == "block"   # another mi355x key is not the recompute key


def test_unknown_mode_raises():
    with pytest.raises(ValueError):
        select_recompute(_cfg(mi355x={"recompute": "bogus"}))


def _clean_env(monkeypatch):
    for k in list(os.environ):
        if k.startswith("PGCA_CFG_") or k in Config.REFERENCE_ENV:
            monkeypatch.delenv(k)


def test_project_default_config_is_unchanged(monkeypatch):
    _clean_env(monkeypatch)
    cfg = Config(os.path.join(ROOT, "configs", "default.yaml"))
    assert cfg.get("hardware.gradient_checkpointing") is None and cfg.get("mi355x.recompute") is None
    assert select_recompute(cfg) == "none"


def test_config_file_and_environment(tmp_path, monkeypatch):
    _clean_env(monkeypatch)
    path = tmp_path / "reference_style.yaml"
    path.write_text(yaml.safe_dump(REFERENCE_STYLE))
    assert select_recompute(Config(str(path))) == "block"
    # the reference-style variable, listed next to the mixed-precision one
    assert Config.REFERENCE_ENV["CAPTION_ALIGNMENT_GRADIENT_CHECKPOINTING"] == "hardware.gradient_checkpointing"
    monkeypatch.setenv("CAPTION_ALIGNMENT_GRADIENT_CHECKPOINTING", "false")
    assert select_recompute(Config(str(path))) == "none"
    monkeypatch.setenv("CAPTION_ALIGNMENT_GRADIENT_CHECKPOINTING", "true")
    assert select_recompute(Config(os.path.join(ROOT, "configs", "default.yaml"))) == "block"
    # this build's generic override form reaches the mi355x key, which wins
    monkeypatch.setenv("PGCA_CFG_MI355X__RECOMPUTE", "mlp")
    assert select_recompute(Config(str(path))) == "mlp"


def test_trainer_calls_the_selector():
    import inspect

    from pgca_amd import trainer
    assert trainer.select_recompute is select_recompute
    src = inspect.getsource(trainer.PreferenceGuidedTrainer)
    assert "select_recompute(config)" in src and src.count("recompute=self.recompute") == 2
