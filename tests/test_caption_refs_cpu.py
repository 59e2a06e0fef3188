"""The references of the caption loss (``caption_refs.py``) proven without a kernel: the float64 restatement of
``pgca_token_nll`` against ``torch.nn.functional.cross_entropy`` and autograd, its bounds against a float32 evaluation, and
the host-side rules that come with the caption objective (config keys, checkpoint rule)."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import caption_refs as C
from step_kernel_refs import r32, ulp32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
F64 = torch.float64


def _case(nrows, nseq, V, seed):
    g = torch.Generator().manual_seed(seed)
    logits = (3.0 * torch.randn(nrows, V, generator=g, dtype=F64)).requires_grad_(True)
    targets = torch.randint(0, V, (nrows,), generator=g)
    seq = torch.sort(torch.randint(0, nseq, (nrows,), generator=g)).values.int()     # rows sorted by sequence
    return logits, targets, seq


@pytest.mark.parametrize("nrows,nseq,limit", [(1, 1, 1), (37, 5, 5), (37, 5, 2), (130, 8, 4), (1030, 16, 9)])
def test_reference_is_cross_entropy_with_ignore_index(nrows, nseq, limit):
    """Mean over the counted rows == CE with the complement set to ignore_index; row_coef == -dLoss/d tok_lp * scale."""
    logits, targets, seq = _case(nrows, nseq, 50, nrows)
    lp = torch.log_softmax(logits, -1)
    tok = lp.gather(1, targets[:, None])[:, 0]
    keep = seq.long() < limit
    want = F.cross_entropy(logits, torch.where(keep, targets, torch.full_like(targets, -100)), ignore_index=-100)
    # the same quantity written on the token log-probs, which is where the kernel's coefficient applies
    via = -tok[keep].mean()
    assert abs(float(via.detach()) - float(want.detach())) <= 1e-12 * abs(float(want.detach()))
    (grad,) = torch.autograd.grad(via, tok)                                            # dLoss / d tok_lp
    want = want.detach()
    # the reference takes the float32 values a kernel would be given
    tok32 = tok.detach().float()
    ref = C.token_nll_ref(tok32, seq, limit, 0.25)
    assert ref["n"] == int(keep.sum()) and ref["metrics"][1] == float(keep.sum()) and ref["metrics"][3] == 1.0
    assert abs(ref["loss"] - float(want)) <= 4 * 2.0 ** -24 * abs(float(want))        # the f32 rounding of tok_lp
    assert abs(ref["metrics"][0] - ref["loss"] * ref["n"]) <= 1e-9 * abs(ref["metrics"][0])
    assert torch.allclose(ref["row_coef"], -grad * r32(0.25), rtol=1e-12, atol=0)
    assert bool((ref["row_coef"][~keep] == 0).all())
    # seq_of_row None counts every row, whatever the limit
    every = C.token_nll_ref(tok32, None, 0, 1.0)
    assert every["n"] == nrows and abs(every["loss"] - float(-tok32.double().mean())) <= 1e-12


def test_seq_limit_split_and_accumulate():
    """The two halves of a split weigh their own token means; accumulate adds onto what is there, counted rows only."""
    logits, targets, seq = _case(200, 10, 30, 7)
    tok = torch.log_softmax(logits, -1).gather(1, targets[:, None])[:, 0].detach().float()
    lo, al = C.token_nll_ref(tok, seq, 4, 1.0), C.token_nll_ref(tok, seq, 10, 1.0)
    keep = seq.long() < 4
    assert lo["n"] == int(keep.sum()) and al["n"] == 200
    assert abs(lo["loss"] - float(-tok.double()[keep].mean())) <= 1e-12
    base = torch.full((200,), 3.0)
    acc = C.token_nll_ref(tok, seq, 4, 0.5, accumulate=True, row_coef_in=base)
    assert torch.equal(acc["row_coef"][~keep], base.double()[~keep])
    assert torch.allclose(acc["row_coef"][keep], torch.full((lo["n"],), 3.0 + 0.5 / lo["n"], dtype=F64), rtol=1e-15)
    assert bool((acc["coef_bound"][~keep] == 0).all()) and bool((acc["coef_bound"][keep] > 0).all())


@pytest.mark.parametrize("bad", [float("-inf"), float("nan")])
def test_non_finite_rules(bad):
    tok = -torch.rand(70) * 9
    tok[33] = bad
    ref = C.token_nll_ref(tok, None, 0, 2.0)
    assert not math.isfinite(ref["loss"]) and ref["metrics"][3] == 0.0
    assert bool((ref["row_coef"] == 0).all()) and bool((ref["coef_bound"] == 0).all())          # accumulate = 0: all zero
    base = torch.full((70,), -7.0)
    acc = C.token_nll_ref(tok, None, 0, 2.0, accumulate=True, row_coef_in=base)
    assert torch.equal(acc["row_coef"], base.double())                                          # accumulate = 1: untouched
    # no counted row: 0/0
    seq = torch.zeros(70, dtype=torch.int32)
    none = C.token_nll_ref(-torch.rand(70), seq, 0, 1.0)
    assert none["n"] == 0 and math.isnan(none["loss"]) and bool((none["row_coef"] == 0).all())
    # the bad row outside the counted set does not matter
    seq[33] = 1
    fine = C.token_nll_ref(tok, seq, 1, 1.0)
    assert math.isfinite(fine["loss"]) and fine["n"] == 69


@pytest.mark.parametrize("nrows", [1, 2, 3, 40, 65, 1025, 4097])
def test_bounds_hold_a_float32_evaluation(nrows):
    """A correctly rounded float32 running sum and division sits inside the loss bound; the float32 quotient
    grad_scale / n sits inside the 1-ulp coefficient bound."""
    g = torch.Generator().manual_seed(nrows)
    tok = -(torch.rand(nrows, generator=g) * 11.0 + 0.01)                 # log-probs of a ~50 k vocabulary: -11 .. 0
    ref = C.token_nll_ref(tok, None, 0, 0.3)
    got = C.token_nll_f32(tok, None, 0)
    err = abs(got - ref["loss"])
    print(f"n={nrows}: f32 loss error {err:.3e}, bound {ref['loss_bound']:.3e}")
    assert err <= ref["loss_bound"]
    c32 = float(torch.tensor(0.3, dtype=torch.float32) / torch.tensor(float(nrows), dtype=torch.float32))
    assert abs(c32 - float(ref["row_coef"][0])) <= float(ref["coef_bound"][0])
    assert float(ref["coef_bound"][0]) == float(ulp32(torch.tensor(c32, dtype=F64)))


def test_masked_ce_is_the_scored_token_mean():
    """``masked_ce`` (the steps' loss on the oracle's logits) == the kernel reference on the oracle's token log-probs."""
    g = torch.Generator().manual_seed(3)
    B, S, V = 3, 9, 17
    logits = torch.randn(B, S, V, generator=g, dtype=F64)
    ids = torch.randint(0, V, (B, S), generator=g)
    mask = (torch.arange(S)[None] < torch.tensor([9, 1, 4])[:, None]).long()        # one caption with ONE real token
    keep = mask[:, 1:] != 0
    tok = torch.log_softmax(logits[:, :-1], -1).gather(2, ids[:, 1:, None])[..., 0][keep]
    assert int(keep[1].sum()) == 0
    assert abs(float(C.masked_ce(logits, ids, mask)) - C.token_nll_ref(tok, None, 0, 1.0)["loss"]) <= 1e-12


# ------------------------------------------------------------------------------------------------ config / checkpoint
def _clean_env(monkeypatch):
    from pgca_amd.config import Config
    for k in list(os.environ):
        if k.startswith("PGCA_CFG_") or k in Config.REFERENCE_ENV:
            monkeypatch.delenv(k)


def test_defaults_select_dpo_without_an_nll_term(monkeypatch):
    from pgca_amd.config import MI355X_DEFAULTS, Config, select_objective
    _clean_env(monkeypatch)
    assert MI355X_DEFAULTS["dpo"]["sft_alpha"] == 0.0
    assert MI355X_DEFAULTS["stage2"] == {"objective": "dpo", "caption_learning_rate": None}
    cfg = Config(os.path.join(ROOT, "configs", "default.yaml"))
    assert select_objective(cfg) == "dpo" and cfg.get("mi355x.dpo.sft_alpha") == 0.0
    assert cfg.get("mi355x.stage2.caption_learning_rate") is None
    # the reference's own configs/default.yaml (a copy of the settings file, tests/golden), parsed unchanged
    ref = Config(os.path.join(GOLDEN, "reference_default.yaml"))
    assert "mi355x" not in ref.config
    assert select_objective(ref) == "dpo" and ref.get("mi355x.dpo.sft_alpha") == 0.0
    assert ref.get("mi355x.stage2.objective") == "dpo"


def test_objective_values(monkeypatch):
    from pgca_amd.config import Config, select_objective
    _clean_env(monkeypatch)
    for mode in ("dpo", "caption", "caption_then_dpo"):
        assert select_objective({"mi355x": {"stage2": {"objective": mode}}}) == mode
    assert select_objective({"mi355x": {"stage2": {"caption_learning_rate": 1e-4}}}) == "dpo"
    with pytest.raises(ValueError, match="mi355x.stage2.objective"):
        select_objective({"mi355x": {"stage2": {"objective": "sft"}}})
    monkeypatch.setenv("PGCA_CFG_MI355X__STAGE2__OBJECTIVE", "caption")
    assert select_objective(Config(os.path.join(ROOT, "configs", "default.yaml"))) == "caption"


def test_checkpoint_without_the_key_is_a_dpo_checkpoint():
    from pgca_amd.config import checkpoint_objective
    assert checkpoint_objective({"epoch": 1, "stage": 2}) == "dpo"
    assert checkpoint_objective({"mi355x_state": {"dropout_step": 3}}) == "dpo"
    assert checkpoint_objective({"mi355x_state": {"objective": "caption"}}) == "caption"
