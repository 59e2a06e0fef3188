"""``evaluation.CaptionEvaluator`` end to end on a tiny model: 8 images, ``max_length`` 12, sampling from a fixed
generator.  What ``evaluate`` returns is what the restatements of tests/eval_refs.py give for the ids
``generate_token_ids`` returns for the same arguments."""
import math

import numpy as np
import pytest
import torch

import eval_refs as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, ML, SEED = 8, 12, 11
GEN = dict(max_length=ML, num_beams=1, do_sample=True, top_p=0.9, temperature=1.0)
LATENCY = ("latency_mean_ms", "latency_median_ms", "latency_p95_ms", "latency_p99_ms")


class ListLoader(list):
    """A loader is anything iterable, as often as asked."""


def gen_kwargs():
    return dict(GEN, generator=torch.Generator(device=DEV).manual_seed(SEED))


@pytest.fixture(scope="module")
def world():
    """The model, the images, the ids it generates in batches of 4 (computed once) and references made from them:
    reference 0 is the generated caption with every third id changed, wrapped in [BOS] .. [EOS]; reference 1 is random;
    reference 2 is absent on even images and empty on odd ones."""
    from pgca_amd.arch import tiny_arch
    from pgca_amd.model import PreferenceGuidedCaptioningModel
    arch = tiny_arch()
    model = PreferenceGuidedCaptioningModel(freeze_vision_backbone=True, arch=arch, dropout=0.0, seed=31, device=DEV)
    g = torch.Generator().manual_seed(5)
    images = torch.randn(N, 3, arch.vit.image, arch.vit.image, generator=g)
    base = arch.gpt.base_vocab
    kw = gen_kwargs()
    raw = [model.generate_token_ids(images[i:i + 4], **kw).cpu() for i in range(0, N, 4)]
    preds = [[t for t in row.tolist() if t < base] for ids in raw for row in ids]
    W = ML + 2
    ref_ids = torch.full((N, 3, W), base, dtype=torch.int64)
    ref_mask = torch.zeros(N, 3, W, dtype=torch.int64)
    refs = []
    for i, p in enumerate(preds):
        near = [t if j % 3 else (t + 1) % base for j, t in enumerate(p)]
        far = torch.randint(0, base, (int(torch.randint(1, ML, (1,), generator=g)),), generator=g).tolist()
        row = [base + 1] + near + [base + 2]                      # [BOS] .. [EOS]: stripped
        ref_ids[i, 0, :len(row)], ref_mask[i, 0, :len(row)] = torch.tensor(row), 1
        ref_ids[i, 1, :len(far)], ref_mask[i, 1, :len(far)] = torch.tensor(far), 1
        refs.append([near, far, None if i % 2 == 0 else []])
    present = torch.ones(N, 3, dtype=torch.bool)
    present[0::2, 2] = False
    return dict(model=model, arch=arch, images=images, raw=raw, preds=preds, refs=refs, ref_ids=ref_ids,
                ref_mask=ref_mask, present=present)


def reference_loader(w, bs):
    return ListLoader({"image": w["images"][i:i + bs], "reference_ids": w["ref_ids"][i:i + bs],
                       "reference_mask": w["ref_mask"][i:i + bs], "reference_present": w["present"][i:i + bs]}
                      for i in range(0, N, bs))


def evaluator(w, **kw):
    from pgca_amd.evaluation import CaptionEvaluator
    return CaptionEvaluator(w["model"], gen_kwargs(), **kw)


def test_evaluate_equals_the_restatements(world):
    w = world
    assert any(w["preds"]) and len(w["preds"]) == N
    w["model"].train(True)
    ev = evaluator(w)
    out = ev.evaluate(reference_loader(w, 4))
    assert w["model"].training is True                            # the training flag is restored
    got_preds = [row[:n].tolist() for row, n in zip(ev.last["pred_ids"], ev.last["length"])]
    assert got_preds == w["preds"]
    assert ev.last["bleu_stats"].tolist() == [E.bleu_stats(p, r) for p, r in zip(w["preds"], w["refs"])]
    want_rows, _ = E.cider_rows(w["preds"], w["refs"])
    err = float(np.abs(ev.last["cider"].numpy() - np.array(want_rows)).max())
    print(f"evaluator: per-image cider max |err| = {err:.3e}; cider = {out['cider']:.6f} bleu_1 = {out['bleu_1']:.6f}")
    assert err <= 1e-9 and abs(out["cider"] - E.cider(w["preds"], w["refs"])) <= 1e-8
    for name, want in E.corpus_bleu(w["preds"], w["refs"]).items():
        assert abs(out[name] - want) <= 1e-12, name
    assert out["bleu_1"] > 0.3                                    # reference 0 keeps two ids of three
    for name, want in E.diversity(w["preds"]).items():
        assert out[name] == want, name
    assert out["num_samples"] == N and out["mean_length"] == sum(len(p) for p in w["preds"]) / N
    assert all(math.isfinite(out[k]) and out[k] > 0.0 for k in LATENCY)
    assert out["latency_mean_ms"] <= out["latency_p99_ms"] * (1 + 1e-12)
    assert "preference_win_rate" not in out and "clip_score" not in out
    w["model"].train(False)
    evaluator(w, measure_latency=False).evaluate(reference_loader(w, 4))
    assert w["model"].training is False


def test_alignment_score_is_the_cosine_of_the_models_towers(world):
    w = world
    m, arch = w["model"], w["arch"]
    m.eval()
    ev = evaluator(w, measure_latency=False)
    out = ev.evaluate(reference_loader(w, 4))
    cos = []
    for b, ids in enumerate(w["raw"]):
        rows = w["preds"][4 * b:4 * b + 4]
        W = ids.shape[1]
        t_ids = torch.full((4, W), arch.gpt.base_vocab, dtype=torch.int64)
        t_mask = torch.zeros(4, W, dtype=torch.int32)
        for i, p in enumerate(rows):
            t_ids[i, :len(p)], t_mask[i, :len(p)] = torch.tensor(p, dtype=torch.int64), 1
        emb = m.vision_encoder(w["images"][4 * b:4 * b + 4].to(DEV))["embeddings"].double().cpu()
        temb = m.text_encoder.engine.forward(t_ids.to(DEV), t_mask.to(DEV), save=False)[2].double().cpu()
        cos.append((emb * temb).sum(1) / (emb.norm(dim=1).clamp_min(1e-12) * temb.norm(dim=1).clamp_min(1e-12)))
    cos = torch.cat(cos)
    bound = 4 * arch.proj_dim * 2.0 ** -24      # as tests/test_mining_kernels_gpu.py bounds pgca_group_cosine
    err = float((ev.last["alignment"] - cos).abs().max())
    print(f"alignment: max |err| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert abs(out["alignment_score"] - float(cos.mean())) <= bound
    assert abs(out["alignment_score_std"] - float(cos.std(unbiased=False))) <= 2 * bound


def test_batch_size_does_not_change_a_score_and_a_corpus_is_reusable(world, monkeypatch):
    """Scoring is per image: batches of 1 and of 4 give identical integers and bitwise-identical CIDEr.  The generated
    ids are held fixed for this (replayed in order), since this is about the scoring and not about the decoder."""
    w = world
    width = max(r.shape[1] for r in w["raw"])
    pad = w["arch"].gpt.base_vocab
    recorded = torch.cat([torch.nn.functional.pad(r, (0, width - r.shape[1]), value=pad) for r in w["raw"]])
    at = [0]

    def replay(images, **kw):
        rows = recorded[at[0]:at[0] + images.shape[0]].to(DEV)
        at[0] += images.shape[0]
        return rows

    monkeypatch.setattr(w["model"], "generate_token_ids", replay)
    results = {}
    for bs in (1, 4):
        at[0] = 0
        ev = evaluator(w, measure_latency=False)
        results[bs] = (ev.evaluate(reference_loader(w, bs)), ev.last)
    (out1, last1), (out4, last4) = results[1], results[4]
    assert torch.equal(last1["bleu_stats"], last4["bleu_stats"]) and torch.equal(last1["length"], last4["length"])
    assert torch.equal(last1["cider"].view(torch.int64), last4["cider"].view(torch.int64))
    for k in out4:
        if not k.startswith("alignment"):
            assert out1[k] == out4[k], k
    # a corpus built once serves every later evaluation
    ev = evaluator(w, measure_latency=False)
    corpus = ev.build_corpus(reference_loader(w, 4))
    assert (corpus.N, corpus.K) == (N, 3) and corpus.n_docs == N
    for _ in range(2):
        at[0] = 0
        assert ev.evaluate(reference_loader(w, 4), corpus=corpus) == out4


def test_the_three_batch_forms(world):
    w = world
    base = w["arch"].gpt.base_vocab
    ids, mask = w["ref_ids"], w["ref_mask"]
    one_ref = [[r[0]] for r in w["refs"]]
    captions = ListLoader({"image": w["images"][i:i + 4], "caption_ids": ids[i:i + 4, 0], "caption_mask": mask[i:i + 4, 0]}
                          for i in range(0, N, 4))
    pairs = ListLoader({"image": w["images"][i:i + 4], "preferred_ids": ids[i:i + 4, 0], "preferred_mask": mask[i:i + 4, 0],
                        "rejected_ids": ids[i:i + 4, 1], "rejected_mask": mask[i:i + 4, 1],
                        "preference_score": torch.ones(4)} for i in range(0, N, 4))
    out_c = evaluator(w, measure_latency=False).evaluate(captions)
    out_p = evaluator(w, measure_latency=False).evaluate(pairs)
    assert not any(k in out_c for k in LATENCY) and not any(k in out_p for k in LATENCY)
    want_bleu = E.corpus_bleu(w["preds"], one_ref)
    for out in (out_c, out_p):
        assert abs(out["cider"] - E.cider(w["preds"], one_ref)) <= 1e-8
        assert all(abs(out[k] - v) <= 1e-12 for k, v in want_bleu.items())
    assert {k: v for k, v in out_p.items() if not k.startswith(("preference", "avg_"))} == out_c
    want = E.preference(w["preds"], [r[0] for r in w["refs"]], [r[1] for r in w["refs"]])
    assert out_p["preference_win_rate"] == want["preference_win_rate"] > 0.5
    for k in ("avg_preferred_similarity", "avg_rejected_similarity", "preference_margin"):
        assert abs(out_p[k] - want[k]) <= 1e-12, k
    assert base not in [t for p in w["preds"] for t in p]


def test_an_image_without_a_reference_is_an_error_that_names_the_count(world):
    w = world
    present = w["present"].clone()
    present[3] = False
    present[6] = False
    loader = ListLoader({"image": w["images"][i:i + 4], "reference_ids": w["ref_ids"][i:i + 4],
                         "reference_mask": w["ref_mask"][i:i + 4], "reference_present": present[i:i + 4]}
                        for i in range(0, N, 4))
    with pytest.raises(ValueError, match=r"2 of 8 images have no reference"):
        evaluator(w, measure_latency=False).evaluate(loader)
