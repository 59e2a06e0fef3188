"""The device-side selection kernels (csrc/select.hip: pgca_select_token, pgca_select_beam_candidates) against the
float64 restatements of tests/select_refs.py, and the surface built on them: ``generate(selection="device")``,
``top_k`` and ``generate_candidates``.

The kernels sum in float32 in their own order, so only DECISIVE inputs are compared (checked on the CPU, in float64):
a row is redrawn when a cumulative mass lies within 1e-5 of 1 - top_p or u * Z within 1e-5 of a CDF step; a beam case
when two of its first K + 1 keys are closer than 1e-4 (float32 log-probabilities and Gumbel noise are good to ~1e-6).
At most 5 % of a case's rows may be redrawn: beyond that the test FAILS.  The seeds below stay under the cap.

Measured on an MI355X (max over the rows of a case, |error| of the log-probability at the chosen token against float64):
see ``test_next_logp_is_as_good_as_torchs_log_softmax``; the figures are recorded in DESIGN.md section 5."""
import pytest
import torch

import select_refs as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 1e-5
FILTERS = ["off", "p0.9", "k1", "k50_p0.8", "kV5_p1e-6"]


def _filter(name, V):
    return {"off": (0, 1.0), "p0.9": (0, 0.9), "k1": (1, 1.0), "k50_p0.8": (50, 0.8), "kV5_p1e-6": (V + 5, 1e-6)}[name]


def _pad4(x):
    """[R, V] -> the [R, V] view of an [R, ld] buffer, ld = V rounded up to 4 (engine._decode_logits), padding poisoned."""
    R, V = x.shape
    buf = torch.full((R, (V + 3) // 4 * 4), float("nan"))
    buf[:, :V] = x
    return buf.to(DEV)[:, :V]


def token_case(V, R, n_prev, sample, filt, seed=None):
    """Decisive inputs of one token-kernel case and their float64 answer (all on the CPU)."""
    top_k, top_p = _filter(filt, V)
    seed = V * 131 + R * 17 + n_prev * 5 + FILTERS.index(filt) if seed is None else seed
    gen = torch.Generator().manual_seed(seed)
    scale = 6.0 if V > 10000 else 3.0
    logits = torch.randn(R, V, generator=gen) * scale
    prev = torch.randint(0, V, (R, max(n_prev, 1)), generator=gen)[:, :n_prev]
    if n_prev >= 2:
        prev[:, -1] = prev[:, 0]                         # a repeated id: the penalty must not compound
    u = torch.rand(R, generator=gen).clamp_(1e-6, 1 - 1e-6) if sample else None
    done = torch.zeros(R, dtype=torch.bool)
    if R > 2:
        done[2] = True
    args = (prev, 1.3, 0.7, top_k, top_p)
    redrawn = 0
    for _ in range(4):
        nxt, nlp, margin = S.select_token(logits, *args, u, done, V + 1)
        bad = (margin < MARGIN).nonzero()[:, 0].tolist()
        if not bad:
            break
        redrawn += len(bad)
        for r in bad:
            logits[r] = torch.randn(V, generator=gen) * scale
            u[r] = float(torch.rand(1, generator=gen).clamp_(1e-6, 1 - 1e-6))
    assert not bad and redrawn <= 0.05 * R, f"{redrawn} of {R} rows redrawn: pick another seed for this case"
    return dict(logits=logits, prev=prev, u=u, done=done, args=args, pad=V + 1, next=nxt, logp=nlp)


def run_token(c):
    from pgca_amd import hip
    hip.load()
    lg = _pad4(c["logits"])
    R, V = c["logits"].shape
    prev = c["prev"].to(DEV)
    rp, T, top_k, top_p = c["args"][1:]
    nxt = torch.full((R,), -7, dtype=torch.int64, device=DEV)
    nlp = torch.full((R,), float("nan"), device=DEV)
    hip.select_token(lg, V, R, prev, prev.shape[1], rp, T, top_k, top_p, None if c["u"] is None else c["u"].to(DEV),
                     c["done"].to(DEV), c["pad"], nxt, nlp)
    return nxt.cpu(), nlp.cpu()


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("n_prev", [0, 7])
@pytest.mark.parametrize("R", [1, 33])
@pytest.mark.parametrize("V", [7, 509, 50260])
def test_sampled_token_equals_the_reference(V, R, n_prev, filt):
    c = token_case(V, R, n_prev, True, filt)
    nxt, nlp = run_token(c)
    assert torch.equal(nxt, c["next"]), (nxt != c["next"]).nonzero()[:, 0].tolist()
    assert float((nlp.double() - c["logp"]).abs().max()) <= 1e-4
    if R > 2:
        assert int(nxt[2]) == c["pad"] and float(nlp[2]) == 0.0
    again = run_token(c)
    assert torch.equal(again[0], nxt) and torch.equal(again[1], nlp)        # bit-identical from run to run


@pytest.mark.parametrize("n_prev", [0, 7])
@pytest.mark.parametrize("R", [1, 33])
@pytest.mark.parametrize("V", [7, 509, 50260])
def test_argmax_token_equals_the_reference(V, R, n_prev):
    c = token_case(V, R, n_prev, False, "off")
    nxt, nlp = run_token(c)
    assert torch.equal(nxt, c["next"])
    assert float((nlp.double() - c["logp"]).abs().max()) <= 1e-4
    if R > 2:
        assert int(nxt[2]) == c["pad"] and float(nlp[2]) == 0.0


def test_penalty_once_per_id_ties_and_all_equal_rows():
    from pgca_amd import hip
    hip.load()
    V = 509
    # row 0: id 5 (+4.0) repeated three times in prev: /2 once leaves 2.0 > 1.9 at id 9; compounding would give 0.5
    # row 1: id 5 (-1.0) repeated: *2 once leaves -2.0 > -2.1 everywhere else; compounding would give -8.0
    x = torch.full((4, V), -3.0)
    x[0, 5], x[0, 9] = 4.0, 1.9
    x[1] = -2.1
    x[1, 5] = -1.0
    x[2] = 0.25                                          # all equal: id 0
    x[3, 100] = x[3, 300] = 1.0                          # an exact tie: the lower id
    prev = torch.tensor([[5, 5, 5, 7], [5, 5, 5, 5], [1, 2, 3, 4], [1, 2, 3, 4]])
    want = S.select_token(x, prev[:, :4], 2.0, 1.0, 0, 1.0, None, None, 0)[0]
    assert want.tolist()[:2] == [5, 5]
    nxt = torch.empty(4, dtype=torch.int64, device=DEV)
    nlp = torch.empty(4, device=DEV)
    hip.select_token(_pad4(x), V, 4, prev.to(DEV), 4, 2.0, 1.0, 0, 1.0, None, None, 0, nxt, nlp)
    assert nxt.tolist()[:2] == [5, 5]
    hip.select_token(_pad4(x), V, 4, prev.to(DEV), 0, 1.0, 1.0, 0, 1.0, None, None, 0, nxt, nlp)
    assert nxt.tolist() == [5, 5, 0, 100]
    # sampling through a compounding penalty would also move mass: top_k 1 after the penalty must still pick id 5
    u = torch.full((4,), 0.5, device=DEV)
    hip.select_token(_pad4(x), V, 4, prev.to(DEV), 4, 2.0, 1.0, 1, 1.0, u, None, 0, nxt, nlp)
    assert nxt.tolist()[:2] == [5, 5]


@pytest.mark.parametrize("V", [7, 509, 50260])
def test_next_logp_is_as_good_as_torchs_log_softmax(V):
    """No fixed tolerance: the kernel's worst error against float64 must be <= 4 x the worst error of torch's own float32
    log_softmax on the GPU on the same rows at the same tokens, + 1e-6.  Both round the same sum; 4 x leaves room for a
    different reduction tree without hiding a wrong normaliser."""
    c = token_case(V, 33, 7, True, "p0.9")
    nxt, nlp = run_token(c)
    assert torch.equal(nxt, c["next"])
    live = ~c["done"]
    ours = float((nlp.double() - c["logp"])[live].abs().max())
    t32 = torch.log_softmax(c["logits"].to(DEV), dim=-1).cpu().gather(1, c["next"].clamp(max=V - 1)[:, None])[:, 0]
    torchs = float((t32.double() - c["logp"])[live].abs().max())
    print(f"next_logp V={V}: kernel max err {ours:.3e}, torch f32 log_softmax max err {torchs:.3e}")
    assert ours <= 4 * torchs + 1e-6, (ours, torchs)


# ------------------------------------------------------------------------------------------------ beam candidates
def beam_case(V, B, nb, noise, warp, tie=False, starve=False, seed=None):
    K = 2 * nb
    seed = V * 7 + B * 31 + nb * 3 + noise if seed is None else seed
    gen = torch.Generator().manual_seed(seed)
    scale = 6.0 if V > 10000 else 3.0
    top_k, top_p = (1, 1.0) if starve else ((50, 0.9) if warp else (0, 1.0))
    redrawn = 0
    for attempt in range(4):
        logits = torch.randn(B * nb, V, generator=gen) * scale
        prev = torch.randint(0, V, (B * nb, 5), generator=gen)
        prev[:, -1] = prev[:, 0]
        bs = -torch.rand(B * nb, generator=gen) * 4
        if tie:                                          # beams 0 and 1 of every item are the same hypothesis
            logits.view(B, nb, V)[:, 1] = logits.view(B, nb, V)[:, 0]
            prev.view(B, nb, 5)[:, 1] = prev.view(B, nb, 5)[:, 0]
            bs.view(B, nb)[:, :2] = 0.0                  # ... and the best-scored ones
        args = (B, nb, prev, 1.2, warp or starve, 0.7, top_k, top_p, bs, K, noise, 1234 + seed)
        score, index, keys = S.beam_candidates(logits, *args)
        gaps = keys[:, :-1] - keys[:, 1:]
        gaps = gaps[torch.isfinite(gaps)]
        if tie and not noise:
            gaps = gaps[gaps != 0]                       # the planted ties are exact in every precision
        if not bool((gaps <= 1e-4).any()):
            break
        redrawn += B
    else:
        raise AssertionError("no decisive beam case found: pick another seed")
    assert redrawn <= 0.05 * B, f"{redrawn} of {B} items redrawn: pick another seed for this case"
    return dict(logits=logits, args=args, score=score, index=index)


def run_beam(c):
    from pgca_amd import hip
    hip.load()
    B, nb, prev, rp, warp, T, top_k, top_p, bs, K, noise, seed = c["args"]
    V = c["logits"].shape[1]
    score = torch.full((B, K), float("nan"), device=DEV)
    index = torch.full((B, K), -7, dtype=torch.int64, device=DEV)
    hip.select_beam_candidates(_pad4(c["logits"]), V, B, nb, prev.to(DEV), prev.shape[1], rp, warp, T, top_k, top_p,
                               bs.to(DEV), K, noise, seed, score, index)
    return score.cpu(), index.cpu()


def _torch_beam_scores(c):
    """What the torch path of _beam_search computes in float32 on the GPU, at the reference's candidates."""
    from pgca_amd.model import CaptionDecoder
    B, nb, prev, rp, warp, T, top_k, top_p, bs = c["args"][:9]
    lp = torch.log_softmax(c["logits"].to(DEV), dim=-1)
    lp = CaptionDecoder._process_scores(lp, prev.to(DEV), rp, warp, T, top_p, top_k)
    acc = (lp + bs.to(DEV)[:, None]).view(B, -1)
    return torch.gather(acc, 1, c["index"].to(DEV)).cpu()


def _check_beam(c):
    score, index = run_beam(c)
    assert torch.equal(index, c["index"])
    fin = torch.isfinite(c["score"])
    assert torch.equal(torch.isfinite(score), fin) and bool((score[~fin] == float("-inf")).all())
    ours = float((score.double() - c["score"])[fin].abs().max())
    torchs = float((_torch_beam_scores(c).double() - c["score"])[fin].abs().max())
    print(f"cand_score: kernel max err {ours:.3e}, torch f32 chain max err {torchs:.3e}")
    assert ours <= 4 * torchs + 1e-6, (ours, torchs)
    again = run_beam(c)
    assert torch.equal(again[1], index) and torch.equal(again[0].view(torch.int32), score.view(torch.int32))


@pytest.mark.parametrize("noise", [0, 1])
@pytest.mark.parametrize("nb", [2, 4])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", [509, 50260])
def test_beam_candidates_equal_the_reference(V, B, nb, noise):
    _check_beam(beam_case(V, B, nb, noise, warp=bool(noise)))


@pytest.mark.parametrize("nb", [2, 4])
def test_beam_ties_go_to_the_lower_flat_index(nb):
    c = beam_case(509, 3, nb, 0, warp=False, tie=True)
    assert bool((c["index"][:, 1] == c["index"][:, 0] + 509).all())      # the same token of beams 0 and 1
    _check_beam(c)


@pytest.mark.parametrize("V,nb", [(509, 2), (509, 4), (50260, 4)])
def test_beam_tail_when_fewer_than_k_keys_are_finite(V, nb):
    c = beam_case(V, 3, nb, 1, warp=True, starve=True)
    assert int(torch.isfinite(c["score"]).sum()) == 3 * nb               # top_k 1: one finite key per beam
    fill = c["index"][0, nb:].tolist()
    assert fill == sorted(fill) and fill[0] <= 1
    _check_beam(c)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def model():
    from pgca_amd.arch import tiny_arch
    from pgca_amd.model import PreferenceGuidedCaptioningModel
    return PreferenceGuidedCaptioningModel(freeze_vision_backbone=True, arch=tiny_arch(), seed=17, device=DEV)


def _images(model, n, seed):
    a = model.arch
    return torch.randn(n, 3, a.vit.image, a.vit.image, generator=torch.Generator().manual_seed(seed))


def test_device_selection_returns_the_torch_paths_ids(model):
    img = _images(model, 5, 31)
    for kw in (dict(num_beams=1, do_sample=False, repetition_penalty=1.1), dict(num_beams=3, do_sample=False)):
        a = model.generate_token_ids(img, max_length=12, selection="torch", **kw)
        b = model.generate_token_ids(img, max_length=12, selection="device", **kw)
        assert a.dtype == b.dtype == torch.int64 and torch.equal(a, b), kw
    with pytest.raises(ValueError, match="selection"):
        model.generate_token_ids(img, max_length=4, selection="bogus")
    with pytest.raises(TypeError):
        model.generate_token_ids(img, max_length=4, num_return_sequences=2)


@pytest.mark.parametrize("beams", [1, 3])
def test_device_sampling_follows_the_generator(model, beams):
    img = _images(model, 3, 4)
    gen = lambda s: torch.Generator(device=DEV).manual_seed(s)  # noqa: E731
    kw = dict(max_length=9, num_beams=beams, do_sample=True, top_p=0.9, temperature=0.8, selection="device")
    a = model.generate_token_ids(img, generator=gen(1), **kw)
    b = model.generate_token_ids(img, generator=gen(1), **kw)
    c = model.generate_token_ids(img, generator=gen(2), **kw)
    assert a.shape == (3, 8) and a.dtype == torch.int64 and torch.equal(a, b) and not torch.equal(a, c)
    assert int(a.max()) < model.arch.dec_vocab and int(a.min()) >= 0


@pytest.mark.parametrize("selection", ["torch", "device"])
def test_top_k_one_sampling_is_greedy(model, selection):
    img = _images(model, 4, 9)
    greedy = model.generate_token_ids(img, max_length=10, num_beams=1, do_sample=False, repetition_penalty=1.1,
                                      selection=selection)
    k1 = model.generate_token_ids(img, max_length=10, num_beams=1, do_sample=True, top_k=1, top_p=1.0, temperature=0.8,
                                  repetition_penalty=1.1, selection=selection,
                                  generator=torch.Generator(device=DEV).manual_seed(5))
    assert torch.equal(greedy, k1)


def test_generate_candidates(model):
    arch, eng = model.arch, model.caption_decoder.engine
    pad, eos = arch.gpt.base_vocab, arch.gpt.base_vocab + 2
    img = _images(model, 2, 13)
    model.train(True)
    ids, logp0, lengths = model.generate_candidates(img, 4, max_length=8, temperature=1.0,
                                                    generator=torch.Generator(device=DEV).manual_seed(3))
    logp = logp0
    assert model.training is True
    model.eval()
    ids2 = model.generate_candidates(img, 4, max_length=8, generator=torch.Generator(device=DEV).manual_seed(3))[0]
    assert model.training is False and torch.equal(ids, ids2)
    Lg = ids.shape[2]
    assert ids.shape == (2, 4, Lg) and 1 <= Lg <= 7 and ids.dtype == torch.int64
    assert logp.shape == (2, 4) and logp.dtype == torch.float32
    assert lengths.shape == (2, 4) and lengths.dtype == torch.int64
    assert int(ids.max()) < arch.dec_vocab
    for b in range(2):
        assert len({tuple(r) for r in ids[b].tolist()}) > 1              # temperature 1.0: not four copies of one caption
    # lengths: up to and including the first [EOS]
    flat = ids.view(8, Lg)
    is_eos = flat == eos
    want_len = torch.where(is_eos.any(1), is_eos.int().argmax(1) + 1, torch.full((8,), Lg, device=flat.device))
    assert torch.equal(lengths.view(8), want_len)
    assert bool((flat[torch.arange(Lg, device=flat.device)[None, :] >= want_len[:, None]] == pad).all())
    # logp: teacher-forced re-scoring of the returned ids (the construction of test_sampling_and_beam_contracts) in
    # float64.  Generated cache-free, the candidates saw exactly the logits the re-scoring sees, so per token the kernel
    # may be off by the next_logp bound only (4 x torch's float32 log_softmax error, measured here, + 1e-6) and by that
    # times the length over the sequence.
    def rescore(flat, want_len):
        pv = eng.prefix_embedding(model.vision_encoder(img)["embeddings"]).repeat_interleave(4, dim=0)
        tot = torch.zeros(8, dtype=torch.float64, device=DEV)
        torch_err = 0.0
        for t in range(flat.shape[1]):
            lg = eng.next_token_logits(pv, flat[:, :t])
            lp64 = torch.log_softmax(lg.double(), dim=-1).gather(1, flat[:, t:t + 1])[:, 0]
            lp32 = torch.log_softmax(lg, dim=-1).gather(1, flat[:, t:t + 1])[:, 0]
            torch_err = max(torch_err, float((lp32.double() - lp64).abs().max()))
            tot += lp64 * (t < want_len)
        return tot, torch_err
    ids, logp, lengths = model.generate_candidates(img, 4, max_length=8, use_cache=False,
                                                   generator=torch.Generator(device=DEV).manual_seed(3))
    tot, torch_err = rescore(ids.view(8, -1), lengths.view(8))
    err = float((logp.view(8).double() - tot).abs().max())
    print(f"generate_candidates: logp max err {err:.3e} over {ids.shape[2]} tokens, torch per-token err {torch_err:.3e}")
    assert err <= (4 * torch_err + 1e-6) * ids.shape[2], (err, torch_err)
    # The K/V-cache decode's logits differ from the cache-free ones by up to 3e-2 (the bound of
    # test_cache_and_cache_free_decoding_agree); a log-softmax moves by at most twice the largest logit change.
    tot, _ = rescore(flat, want_len)
    assert float((logp0.view(8).double() - tot).abs().max()) <= 2 * 3e-2 * Lg
