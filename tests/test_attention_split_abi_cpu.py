"""C boundary of the split attention backward (``pgca_attention_bwd_split``), the ViT-L/14@336 geometry and the engine's
sequence-length ceiling, no GPU needed: header prototype <-> export <-> ctypes signature, and the argument checks that
run before any launch."""
import ctypes
import os
import re

import pytest
import torch  # noqa: F401  (loads libamdhip64 first, as the product does)

from pgca_amd import REPO_ROOT, abi, hip


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(hip.LIB_PATH):
        from pgca_amd import build
        build.build()
    return hip.load()


def header():
    return open(os.path.join(REPO_ROOT, "include", "pgca_hip.h")).read()


def prototype(name):
    assert abi.PROTOTYPES[name].ret == "int", f"{name} has no status-returning prototype in pgca_hip.h"
    return [f"{t} {n}" for t, n in abi.PROTOTYPES[name].params]


def test_split_entry_is_declared_exported_and_bound(lib):
    params = prototype("pgca_attention_bwd_split")
    assert params == prototype("pgca_attention_bwd"), "the split entry takes pgca_attention_bwd's argument list"
    assert "pgca_attention_bwd_split" in hip.EXPORTS and hasattr(lib, "pgca_attention_bwd_split")
    sig = hip._SIGS["pgca_attention_bwd_split"]
    assert sig == hip._SIGS["pgca_attention_bwd"] and len(sig) == len(params)
    assert lib.pgca_attention_bwd_split.argtypes == sig and lib.pgca_attention_bwd_split.restype is ctypes.c_int
    assert callable(hip.attention_bwd_split)
    import inspect
    assert inspect.signature(hip.attention_bwd_split) == inspect.signature(hip.attention_bwd)


def test_limits_in_the_header_and_the_abi_version_stay(lib):
    h = header()
    assert re.search(r"#define\s+PGCA_ATTN_SPLIT_MAX_S\s+1024\b", h)
    assert re.search(r"#define\s+PGCA_ATTN_MAX_S\s+512\b", h), "the one-pass entry keeps its limit"
    assert lib.pgca_version() == hip.ABI_VERSION == 306   # additive: no signature or struct changed


def _call(lib, qkv=0x1000, out=0x2000, dout=0x3000, lse=0x4000, dqkv=0x5000, B=2, S=640, heads=2):
    """Fake, aligned operand addresses: validation reads no memory, and every call here must be refused."""
    return lib.pgca_attention_bwd_split(qkv, out, dout, lse, None, B, S, heads, 1, dqkv, 0, 0, 1.0, None, None)


def test_arguments_are_checked_before_any_launch(lib):
    for null in ("qkv", "out", "dout", "lse", "dqkv"):
        assert _call(lib, **{null: None}) == -1, null
        assert b"pgca_attention_bwd_split" in lib.pgca_last_error()
    assert _call(lib, S=1025) == -1
    err = lib.pgca_last_error()
    assert b"1024" in err and b"S=1025" in err, err
    assert _call(lib, S=0) == -1
    assert _call(lib, B=0) == -1
    assert _call(lib, B=65536) == -1 and b"65535" in lib.pgca_last_error()
    assert _call(lib, heads=0) == -1


def test_vit_l14_336_is_in_the_zoo():
    from pgca_amd.arch import VIT_ZOO, make_arch
    a = VIT_ZOO["openai/clip-vit-large-patch14-336"]
    assert (a.hidden, a.layers, a.heads, a.mlp, a.patch, a.image) == (1024, 24, 16, 4096, 14, 336)
    assert a.grid == 24 and a.tokens == 577 and a.patch_dim == 588
    arch = make_arch("openai/clip-vit-large-patch14-336", "gpt2-medium")
    assert arch.vit is a and arch.gpt.n_pos == 1024


def test_engine_ceiling_and_dispatch(monkeypatch):
    from pgca_amd import engine
    assert engine.ATTN_BWD_MAX_S == 1024
    calls = []
    monkeypatch.setattr(hip, "attention_bwd", lambda *a, **k: calls.append(("onepass", a[6])))
    monkeypatch.setattr(hip, "attention_bwd_split", lambda *a, **k: calls.append(("split", a[6])))
    for S in (1, 128, 512, 513, 577, 1024):
        engine.attention_backward(None, None, None, None, None, 1, S, 1, True, None)
    assert calls == [("onepass", 1), ("onepass", 128), ("onepass", 512), ("split", 513), ("split", 577), ("split", 1024)]


def test_train_script_image_size_follows_the_tower():
    import importlib.util
    spec = importlib.util.spec_from_file_location("pgca_train_script", os.path.join(REPO_ROOT, "scripts", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.synthetic_image_size(None, 336, "openai/clip-vit-large-patch14-336") == 336
    assert mod.synthetic_image_size(224, 224, "openai/clip-vit-base-patch32") == 224
    with pytest.raises(ValueError, match="336"):
        mod.synthetic_image_size(224, 336, "openai/clip-vit-large-patch14-336")
