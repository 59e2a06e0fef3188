"""Pins tests/beam_refs.py - the restatement the GPU tests of the selection bans, ``pgca_beam_step`` and the new
``generate`` arguments compare against - to transformers itself: the ban masks against HF's own logits processors, and
the restated beam loop, fed the same logits, against ``GPT2LMHeadModel.generate(inputs_embeds=...)``.

The model is a tiny random GPT-2 built here (nothing is downloaded).  A plain random model never emits [EOS], and then
none of the length / stopping arguments changes anything; its LM head is therefore replaced by one with larger weights
and a bias on the [EOS] logit, so [EOS] competes at every step.  Every case asserts that its argument changes the
output of the same call without it."""
import os

import pytest
import torch

import beam_refs as R

transformers = pytest.importorskip("transformers")
from transformers import GPT2Config, GPT2LMHeadModel  # noqa: E402
from transformers.generation.logits_process import (MinLengthLogitsProcessor,  # noqa: E402
                                                    MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor,
                                                    SuppressTokensLogitsProcessor)

V, EOS, PAD = 61, 60, 59


# ------------------------------------------------------------------------------------------------ processors
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("n_prev", [0, 1, 2, 9])
def test_ngram_bans_equal_hfs_processor(n, n_prev):
    gen = torch.Generator().manual_seed(100 * n + n_prev)
    prev = torch.randint(0, 5, (6, n_prev), generator=gen)          # 5 ids: repeats are certain at 9
    if n_prev == 9 and n > 1:
        prev[0] = torch.tensor([1, 2, 3, 1, 2, 4, 0, 1, 2])[:9]     # (1, 2) matched twice: bans 3 and 4 for n = 3
        if n == 2:
            prev[1] = torch.tensor([2, 3, 0, 2, 4, 1, 1, 0, 2])     # 2 -> {3, 4}
    scores = torch.randn(6, V, generator=gen)
    want = torch.isinf(NoRepeatNGramLogitsProcessor(n)(prev, scores.clone()))
    got = R.ban_mask(prev, V, n)
    assert torch.equal(got, want)
    if n_prev < n - 1 or n_prev == 0:
        assert not bool(got.any())
    if n_prev == 9 and n == 3:
        assert got[0].nonzero()[:, 0].tolist() == [3, 4]
    if n_prev == 9 and n == 1:
        assert got[0].nonzero()[:, 0].tolist() == sorted(set(prev[0].tolist()))
    # the processed scores: -inf where banned, untouched elsewhere
    s = R.process(scores, prev, 1.0, False, no_repeat_ngram_size=n)
    assert torch.equal(torch.isinf(s), want) and torch.equal(s[~want], scores.double()[~want])


@pytest.mark.parametrize("step", [0, 2, 3, 5])
def test_min_length_and_suppress_bans_equal_hfs_processors(step):
    gen = torch.Generator().manual_seed(step)
    prev = torch.randint(0, V, (4, step), generator=gen)
    scores = torch.randn(4, V, generator=gen)
    dev = torch.device("cpu")
    for min_new in (0, 3, 5):
        want = scores.clone()
        if min_new:
            want = MinLengthLogitsProcessor(min_new, EOS, device=dev)(prev, want)
            want = MinNewTokensLengthLogitsProcessor(0, min_new, EOS, device=dev)(prev, want)
        want = SuppressTokensLogitsProcessor([7, 11], device=dev)(prev, want)
        ids = R.min_length_ban_ids(step, EOS, min_new, [7, 11, V + 3, -1])   # out-of-range ids are ignored
        got = R.process(scores, prev, 1.0, False, ban_ids=ids)
        assert torch.equal(torch.isinf(got), torch.isinf(want))
        assert bool(torch.isinf(got[:, EOS]).all()) == (step < min_new)


def test_a_ban_dominates_the_repetition_penalty_and_the_warpers_see_it():
    scores = torch.tensor([[2.0, 1.0, -1.0, 0.5]])
    prev = torch.tensor([[0, 2]])
    s = R.process(scores, prev, 2.0, True, 1.0, 2, 1.0, no_repeat_ngram_size=1)
    assert torch.isinf(s[0, [0, 2]]).all()                          # seen ids: penalised, then banned
    assert s[0, 1] == 1.0 and s[0, 3] == 0.5                        # top-k 2 keeps the two that are left


# ------------------------------------------------------------------------------------------------ beam loop vs HF
@pytest.fixture(scope="module")
def hf():
    torch.manual_seed(3)
    cfg = GPT2Config(vocab_size=V, n_positions=32, n_embd=32, n_layer=2, n_head=2, bos_token_id=EOS, eos_token_id=EOS,
                     pad_token_id=PAD, tie_word_embeddings=False, attn_pdrop=0.0, embd_pdrop=0.0, resid_pdrop=0.0)
    model = GPT2LMHeadModel(cfg).eval()
    head = torch.nn.Linear(32, V, bias=True)
    with torch.no_grad():
        head.weight.normal_(0.0, 0.35)
        head.bias.zero_()
        head.bias[EOS] = 5.0
    model.lm_head = head
    prefix = torch.randn(3, 1, 32)
    return model, prefix


def _hf_generate(hf, **kw):
    model, prefix = hf
    kw.setdefault("max_length", 12)
    out = model.generate(inputs_embeds=prefix, num_beams=3, do_sample=False, pad_token_id=PAD, eos_token_id=EOS,
                         return_dict_in_generate=True, output_scores=True, **kw)
    return out.sequences, out.sequences_scores


def _ours(hf, max_length=12, max_new_tokens=None, min_length=0, min_new_tokens=None, num_return_sequences=1,
          suppress_tokens=(), **kw):
    model, prefix = hf
    nb = 3
    L = max_length - 1 if max_new_tokens is None else max_new_tokens
    min_new = max(min_length - 1, 0) if min_new_tokens is None else min_new_tokens
    pre = prefix.repeat_interleave(nb, dim=0)

    @torch.no_grad()
    def logits_fn(prev):
        emb = torch.cat([pre, model.transformer.wte(prev)], dim=1)
        return model(inputs_embeds=emb).logits[:, -1]

    seq, sc, glen = R.beam_search(logits_fn, 3, nb, L, PAD, EOS, min_new=min_new, suppress=suppress_tokens, **kw)
    n = num_return_sequences
    out_len = max(1, int(glen[:, :n].max()))
    return seq[:, :n, :out_len].reshape(3 * n, out_len), sc[:, :n].reshape(-1)


CASES = {
    # [EOS] ends these sequences before an id could repeat: a minimum length keeps them running
    "no_repeat_ngram_size_1": (dict(no_repeat_ngram_size=1, min_new_tokens=8),
                               dict(no_repeat_ngram_size=1, min_new_tokens=8)),
    "no_repeat_ngram_size_2": (dict(no_repeat_ngram_size=2, min_new_tokens=11),
                               dict(no_repeat_ngram_size=2, min_new_tokens=11)),
    "min_length": (dict(min_length=7), dict(min_length=7)),
    "min_new_tokens": (dict(min_new_tokens=5), dict(min_new_tokens=5)),
    "max_new_tokens": (dict(max_new_tokens=2, min_new_tokens=2), dict(max_new_tokens=2, min_new_tokens=2)),
    "length_penalty_0": (dict(length_penalty=0.0), dict(length_penalty=0.0)),
    "length_penalty_2": (dict(length_penalty=2.0), dict(length_penalty=2.0)),
    "early_stopping_true": (dict(early_stopping=True), dict(early_stopping=True)),
    "early_stopping_never": (dict(early_stopping="never", length_penalty=2.0),
                             dict(early_stopping="never", length_penalty=2.0)),
    "num_return_sequences": (dict(num_return_sequences=2), dict(num_return_sequences=2)),
    "suppress_tokens": (dict(suppress_tokens=[EOS]), dict(suppress_tokens=[EOS])),
}
# what each case is compared with to show that its argument matters
BASELINE = {"early_stopping_never": dict(length_penalty=2.0), "max_new_tokens": dict(min_new_tokens=2),
            "no_repeat_ngram_size_1": dict(min_new_tokens=8), "no_repeat_ngram_size_2": dict(min_new_tokens=11)}


def _same(a, b):
    return a[0].shape == b[0].shape and torch.equal(a[0], b[0]) and torch.allclose(a[1], b[1], rtol=1e-5, atol=1e-6)


def test_default_arguments_equal_hf(hf):
    seq, sc = _hf_generate(hf)
    got = _ours(hf)
    assert torch.equal(got[0], seq) and torch.allclose(got[1], sc, rtol=1e-5, atol=1e-6)
    assert bool((seq == EOS).any())                                 # [EOS] does compete


@pytest.mark.parametrize("name", sorted(CASES))
def test_beam_loop_equals_hf_generate(hf, name):
    hf_kw, our_kw = CASES[name]
    seq, sc = _hf_generate(hf, **hf_kw)
    got = _ours(hf, **our_kw)
    assert got[0].shape == seq.shape and torch.equal(got[0], seq), (got[0], seq)
    assert torch.allclose(got[1], sc, rtol=1e-5, atol=1e-6), (got[1], sc)
    base = _ours(hf, **BASELINE.get(name, {}))
    assert not _same(got, base), f"{name} changes nothing on this model: the case is vacuous"


def test_reading_the_stop_flag_every_8_steps_changes_nothing(hf):
    for kw in (dict(), dict(early_stopping=True), dict(early_stopping="never", length_penalty=2.0)):
        assert _same(_ours(hf, eos_check=8, **kw), _ours(hf, **kw)), kw


# ------------------------------------------------------------------------------------------------ config helper
def test_generate_kwargs_from_the_shipped_config():
    from pgca_amd import REPO_ROOT
    from pgca_amd.config import Config, generate_kwargs
    kw = generate_kwargs(Config(os.path.join(REPO_ROOT, "configs", "default.yaml")))
    assert kw == dict(max_length=128, num_beams=4, temperature=0.8, do_sample=True, top_p=0.9, repetition_penalty=1.1,
                      length_penalty=1.0)
    assert type(kw["length_penalty"]) is float and type(kw["max_length"]) is int and kw["do_sample"] is True
    with pytest.raises(ValueError, match="bad_words_ids"):
        generate_kwargs({"evaluation": {"generate_config": {"bad_words_ids": [[1]]}}})
    with pytest.raises(KeyError):
        generate_kwargs({"evaluation": {}})
