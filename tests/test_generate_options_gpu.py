"""The generation arguments ``CaptionDecoder.generate`` takes beyond the reference's defaults - ``no_repeat_ngram_size``,
``min_length`` / ``min_new_tokens``, ``max_new_tokens``, ``suppress_tokens``, ``length_penalty``, ``early_stopping``,
``return_scores`` - end to end on the tiny model of test_select_gpu.py: ``selection="device"`` (the ``_ex`` selection
kernels and ``pgca_beam_step``) against ``selection="torch"``, both against the beam loop of tests/beam_refs.py, which
test_beam_refs_cpu.py pins to transformers' ``generate``.

Random weights never emit the tokenizer's [EOS], and then the length and stopping arguments change nothing: the tests
pass an ``eos_token_id`` the model does emit - the id default beam search puts third in its first caption."""
import pytest
import torch

import beam_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ML = 12                                                          # max_length: 11 generated tokens


@pytest.fixture(scope="module")
def model():
    from pgca_amd.arch import tiny_arch
    from pgca_amd.model import PreferenceGuidedCaptioningModel
    return PreferenceGuidedCaptioningModel(freeze_vision_backbone=True, arch=tiny_arch(), seed=17, device=DEV)


@pytest.fixture(scope="module")
def img(model):
    a = model.arch
    return torch.randn(5, 3, a.vit.image, a.vit.image, generator=torch.Generator().manual_seed(31))


@pytest.fixture(scope="module")
def eos(model, img):
    ids = model.generate_token_ids(img, max_length=ML, num_beams=3, do_sample=False)
    return int(ids[0, 2])


BEAM = dict(num_beams=3, do_sample=False)
OPTIONS = [
    dict(no_repeat_ngram_size=1, min_new_tokens=8),
    dict(no_repeat_ngram_size=2, min_new_tokens=11),
    dict(no_repeat_ngram_size=3, min_new_tokens=11, repetition_penalty=1.0),
    dict(min_length=7),
    dict(min_new_tokens=5),
    dict(max_new_tokens=4),
    dict(max_new_tokens=3, min_new_tokens=3),
    dict(suppress_tokens=[0, 1, 2, 3]),
    dict(length_penalty=0.0),
    dict(length_penalty=2.0),
    dict(early_stopping=True),
    dict(early_stopping="never", length_penalty=2.0),
    dict(early_stopping="never", length_penalty=0.0),
]


def _restated(model, img, eos, nb=3, max_length=ML, max_new_tokens=None, min_length=0, min_new_tokens=None,
              suppress_tokens=(), repetition_penalty=1.1, eos_check=8, **kw):
    """The beam loop of beam_refs.py on this model's cache-free logits."""
    eng = model.caption_decoder.engine
    B = img.shape[0]
    model.eval()
    pv = eng.prefix_embedding(model.vision_encoder(img)["embeddings"].to(DEV, torch.float32).contiguous())
    pvr = pv.repeat_interleave(nb, dim=0)
    L = max_length - 1 if max_new_tokens is None else max_new_tokens
    min_new = max(min_length - 1, 0) if min_new_tokens is None else min_new_tokens
    fn = lambda prev: eng.next_token_logits(pvr, prev.to(DEV)).float().cpu()  # noqa: E731
    seq, sc, glen = R.beam_search(fn, B, nb, L, model.arch.gpt.base_vocab, eos, repetition_penalty,
                                  min_new=min_new, suppress=suppress_tokens, eos_check=eos_check, **kw)
    return seq[:, 0, :max(1, int(glen[:, 0].max()))], sc[:, 0]


def test_default_arguments_return_what_the_old_bookkeeping_returned(model, img):
    """The restated loop with default options is the torch bookkeeping ``_beam_search`` had before ``pgca_beam_step``:
    both paths must still return its ids, with the tokenizer's own [EOS] and with one that occurs."""
    for eos_id in (None, int(model.generate_token_ids(img, max_length=ML, **BEAM)[0, 2])):
        kw = {} if eos_id is None else dict(eos_token_id=eos_id)
        want = _restated(model, img, model.arch.gpt.base_vocab + 2 if eos_id is None else eos_id)[0]
        for selection in ("torch", "device"):
            got = model.generate_token_ids(img, max_length=ML, use_cache=False, selection=selection, **BEAM, **kw)
            assert torch.equal(got.cpu(), want), (selection, eos_id)


@pytest.mark.parametrize("use_cache", [True, False])
@pytest.mark.parametrize("opt", OPTIONS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_device_selection_equals_the_torch_path_for_every_argument(model, img, eos, opt, use_cache):
    kw = dict(max_length=ML, eos_token_id=eos, use_cache=use_cache, return_scores=True, **BEAM, **opt)
    a, sa = model.generate_token_ids(img, selection="torch", **kw)
    b, sb = model.generate_token_ids(img, selection="device", **kw)
    assert a.dtype == b.dtype == torch.int64 and torch.equal(a, b)
    assert sa.shape == sb.shape == (5,) and sa.dtype == sb.dtype == torch.float32
    assert torch.allclose(sa, sb, rtol=1e-5, atol=1e-5), (sa, sb)
    if not use_cache:                                            # ... and both equal HF's rules restated
        want, want_sc = _restated(model, img, eos, **opt)
        assert torch.equal(a.cpu(), want) and torch.allclose(sa.cpu(), want_sc, rtol=1e-5, atol=1e-5)
    plain = model.generate_token_ids(img, selection="device", **{k: v for k, v in kw.items() if k != "return_scores"})
    assert torch.equal(plain, b)


@pytest.mark.parametrize("selection", ["torch", "device"])
def test_greedy_and_sampling_take_the_ban_options(model, img, eos, selection):
    base = model.arch.gpt.base_vocab
    kw = dict(max_length=ML, eos_token_id=eos, num_beams=1, selection=selection)
    opts = dict(no_repeat_ngram_size=2, min_new_tokens=6, suppress_tokens=[4, 5])
    g = model.generate_token_ids(img, do_sample=False, **kw, **opts)
    if selection == "device":
        assert torch.equal(g, model.generate_token_ids(img, do_sample=False, **dict(kw, selection="torch"), **opts))
        assert torch.equal(g, model.generate_token_ids(img, do_sample=False, use_cache=False, **kw, **opts))
    s = model.generate_token_ids(img, do_sample=True, top_p=0.9, temperature=1.5,
                                 generator=torch.Generator(device=DEV).manual_seed(3), **kw, **opts)
    for ids in (g, s):
        for row in ids.tolist():
            n = row.index(eos) + 1 if eos in row else len(row)
            assert n >= 6 and 4 not in row[:n] and 5 not in row[:n]
            grams = list(zip(row[:n], row[1:n]))
            assert len(grams) == len(set(grams)), row
            assert all(t == base for t in row[n:])


def test_no_repeated_bigram_and_no_early_eos_in_beam_search(model, img, eos):
    for selection in ("torch", "device"):
        for sample in (False, True):
            ids = model.generate_token_ids(img, max_length=ML, eos_token_id=eos, num_beams=3, do_sample=sample,
                                           no_repeat_ngram_size=2, min_new_tokens=7, selection=selection,
                                           generator=torch.Generator(device=DEV).manual_seed(1))
            for row in ids.tolist():
                n = row.index(eos) + 1 if eos in row else len(row)
                assert n >= 7, row
                grams = list(zip(row[:n], row[1:n]))
                assert len(grams) == len(set(grams)), row


@pytest.mark.parametrize("selection", ["torch", "device"])
def test_the_read_back_cadence_changes_nothing(model, img, eos, selection):
    dec = model.caption_decoder
    for es, lp in ((False, 1.0), (True, 1.0), ("never", 2.0), ("never", 0.0)):
        kw = dict(max_length=ML, eos_token_id=eos, early_stopping=es, length_penalty=lp, return_scores=True,
                  selection=selection, **BEAM)
        outs = []
        for check in (1, 8):
            dec.EOS_CHECK = check
            try:
                outs.append(model.generate_token_ids(img, **kw))
            finally:
                del dec.EOS_CHECK                                # back to the class attribute
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (es, lp)


def test_generate_candidates_takes_the_ban_options(model, img):
    eos = model.arch.gpt.base_vocab + 2
    ids, logp, lengths = model.generate_candidates(img[:2], 3, max_length=9, no_repeat_ngram_size=1, min_length=5,
                                                   suppress_tokens=[7], temperature=1.5,
                                                   generator=torch.Generator(device=DEV).manual_seed(2))
    assert ids.shape[:2] == (2, 3) and bool(torch.isfinite(logp).all())
    for row, n in zip(ids.view(6, -1).tolist(), lengths.view(6).tolist()):
        assert len(set(row[:n])) == n and 7 not in row[:n] and eos not in row[:4]


def test_argument_errors(model, img):
    gen = lambda **kw: model.generate_token_ids(img, max_length=6, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="return_scores"):
        gen(num_beams=1, do_sample=False, return_scores=True)
    with pytest.raises(ValueError, match="early_stopping"):
        gen(early_stopping="sometimes")
    with pytest.raises(ValueError, match="min_new_tokens"):
        gen(min_new_tokens=9)
    with pytest.raises(ValueError, match="max_new_tokens"):
        gen(max_new_tokens=0)
    with pytest.raises(TypeError, match="bad_words_ids"):
        gen(bad_words_ids=[[1, 2]])
    assert gen(max_new_tokens=9, num_beams=2, do_sample=False).shape[1] <= 9   # max_new_tokens wins over max_length
    assert gen(min_length=6, num_beams=2, do_sample=False).shape == (5, 5)     # the prefix is one of the six positions
