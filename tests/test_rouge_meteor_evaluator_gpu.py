"""``rouge1`` / ``rouge2`` / ``rougeL`` / ``meteor`` of ``evaluation.CaptionEvaluator`` end to end on a tiny model: 8 images,
2 references, ``max_length`` 12, sampling from a fixed generator.  The four keys are what the restatements of
tests/rouge_meteor_refs.py give for the ids the evaluator scored (``last["pred_ids"]``) and the loader's stripped
references, within 1e-12 absolute: each is a mean of 8 float64 values in [0, 1] formed from exact integers, so product and
restatement differ by a few roundings of 1e-16.  The older keys, the single read-back and the absence of a synchronise
are unchanged."""
import pytest
import torch

import rouge_meteor_refs as R
from test_eval_trainer_gpu import _run as run_trainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, ML, SEED = 8, 12, 11
GEN = dict(max_length=ML, num_beams=1, do_sample=True, top_p=0.9, temperature=1.0)
NEW = {"rouge1", "rouge2", "rougeL", "meteor"}


class ListLoader(list):
    """A loader is anything iterable, as often as asked."""


def gen_kwargs():
    return dict(GEN, generator=torch.Generator(device=DEV).manual_seed(SEED))


@pytest.fixture(scope="module")
def world():
    """The model, the images, the ids it generates in batches of 4 (computed once, replayed afterwards so that every
    evaluation scores the same captions) and two references made from them: reference 0 is the generated caption with
    every third id changed and its halves swapped, in [BOS] .. [EOS], absent on image 2; reference 1 is the caption
    reversed on even images and random on odd ones."""
    from pgca_amd.arch import tiny_arch
    from pgca_amd.model import PreferenceGuidedCaptioningModel
    arch = tiny_arch()
    model = PreferenceGuidedCaptioningModel(freeze_vision_backbone=True, arch=arch, dropout=0.0, seed=31, device=DEV)
    g = torch.Generator().manual_seed(5)
    images = torch.randn(N, 3, arch.vit.image, arch.vit.image, generator=g)
    base = arch.gpt.base_vocab
    kw = gen_kwargs()
    raw = [model.generate_token_ids(images[i:i + 4], **kw).cpu() for i in range(0, N, 4)]
    width = max(r.shape[1] for r in raw)
    recorded = torch.cat([torch.nn.functional.pad(r, (0, width - r.shape[1]), value=base) for r in raw])
    preds = [[t for t in row.tolist() if t < base] for row in recorded]
    W = ML + 2
    ref_ids = torch.full((N, 2, W), base, dtype=torch.int64)
    ref_mask = torch.zeros(N, 2, W, dtype=torch.int64)
    present = torch.ones(N, 2, dtype=torch.bool)
    present[2, 0] = False
    refs = []
    for i, p in enumerate(preds):
        near = [t if j % 3 else (t + 1) % base for j, t in enumerate(p)]
        near = near[len(near) // 2:] + near[:len(near) // 2]
        other = p[::-1] if i % 2 == 0 else torch.randint(0, base, (ML - 3,), generator=g).tolist()
        row = [base + 1] + near + [base + 2]                      # [BOS] .. [EOS]: stripped
        ref_ids[i, 0, :len(row)], ref_mask[i, 0, :len(row)] = torch.tensor(row), 1
        ref_ids[i, 1, :len(other)], ref_mask[i, 1, :len(other)] = torch.tensor(other, dtype=torch.int64), 1
        refs.append([near if present[i, 0] else None, other])
    return dict(model=model, arch=arch, images=images, recorded=recorded, preds=preds, refs=refs, ref_ids=ref_ids,
                ref_mask=ref_mask, present=present)


def loader(w, bs):
    return ListLoader({"image": w["images"][i:i + bs], "reference_ids": w["ref_ids"][i:i + bs],
                       "reference_mask": w["ref_mask"][i:i + bs], "reference_present": w["present"][i:i + bs]}
                      for i in range(0, N, bs))


@pytest.fixture
def replayed(world, monkeypatch):
    """``world`` with generation replaced by the recorded ids, in loader order; ``rewind()`` starts over."""
    at = [0]

    def replay(images, **kw):
        rows = world["recorded"][at[0]:at[0] + images.shape[0]].to(DEV)
        at[0] += images.shape[0]
        return rows

    monkeypatch.setattr(world["model"], "generate_token_ids", replay)
    return dict(world, rewind=lambda: at.__setitem__(0, 0))


def evaluate(w, bs, corpus=None, **kw):
    from pgca_amd.evaluation import CaptionEvaluator
    w["rewind"]()
    ev = CaptionEvaluator(w["model"], gen_kwargs(), measure_latency=False, **kw)
    return ev.evaluate(loader(w, bs), corpus=corpus), ev


def test_the_new_keys_equal_the_restatements(replayed):
    w = replayed
    out, ev = evaluate(w, 4)
    preds = [row[:n].tolist() for row, n in zip(ev.last["pred_ids"], ev.last["length"])]
    assert preds == w["preds"] and any(len(p) >= 4 for p in preds)
    assert ev.last["rouge_stats"].tolist() == [R.rouge_stats(p, r) for p, r in zip(preds, w["refs"])]
    assert ev.last["meteor_stats"].tolist() == [R.meteor_stats(p, r) for p, r in zip(preds, w["refs"])]
    assert ev.last["rouge_stats"][2, 5] == 1                      # image 2 is scored against its second reference
    want = dict(R.rouge(preds, w["refs"]), meteor=R.meteor(preds, w["refs"]))
    assert set(want) == NEW
    for name, value in want.items():
        print(f"evaluator: {name} = {out[name]:.12f}, restatement {value:.12f}, |diff| = {abs(out[name] - value):.3e}")
        assert abs(out[name] - value) <= 1e-12, name
    # reference 0 keeps two ids of three but in swapped halves: order-free overlap is high, the order-sensitive scores
    # stay below it
    assert out["rouge1"] > 0.3 and out["rougeL"] <= out["rouge1"] and 0.0 < out["meteor"] < 1.0


def test_batch_size_does_not_change_a_score(replayed):
    (out1, ev1), (out4, ev4) = evaluate(replayed, 1), evaluate(replayed, 4)
    assert torch.equal(ev1.last["rouge_stats"], ev4.last["rouge_stats"])
    assert torch.equal(ev1.last["meteor_stats"], ev4.last["meteor_stats"])
    for name in NEW:
        assert out1[name] == out4[name], name


def test_the_older_keys_the_read_back_and_the_synchronise_count_are_unchanged(replayed, monkeypatch):
    """The same evaluator with and without the two new launches returns the same value under every older key; with a
    corpus at hand one evaluation reads back twice (the packed per-image buffer and ``last["pred_ids"]``), as before
    the two kernels were added, and ``measure_latency=False`` synchronises nowhere."""
    from pgca_amd import hip
    w = replayed
    _, ev = evaluate(w, 4)
    corpus = ev.build_corpus(loader(w, 4))
    counts = {"cpu": 0, "sync": 0}
    tensor_cpu, synchronize = torch.Tensor.cpu, torch.cuda.synchronize

    def counted_cpu(self, *a, **kw):
        counts["cpu"] += 1 if self.is_cuda else 0
        return tensor_cpu(self, *a, **kw)

    def counted_sync(*a, **kw):
        counts["sync"] += 1
        return synchronize(*a, **kw)

    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", counted_cpu)
        mp.setattr(torch.cuda, "synchronize", counted_sync)
        out, _ = evaluate(w, 4, corpus=corpus)
    assert counts == {"cpu": 2, "sync": 0}
    with monkeypatch.context() as mp:
        mp.setattr(hip, "rouge_stats", lambda *a: None)
        mp.setattr(hip, "meteor_stats", lambda *a: None)
        without, _ = evaluate(w, 4, corpus=corpus)
    assert set(out) == set(without) and NEW <= set(out)
    older = set(out) - NEW
    assert {"bleu_1", "bleu_2", "bleu_3", "bleu_4", "cider", "diversity_1", "diversity_2", "unique_caption_ratio", "alignment_score",
            "alignment_score_std", "num_samples", "mean_length"} == older
    for name in older:
        assert out[name] == without[name], name
    assert all(without[name] == 0.0 for name in NEW)              # the zeroed buffers: nothing else feeds the new keys


def test_the_trainer_returns_the_new_keys(tmp_path):
    _, out = run_trainer(tmp_path, **{"mi355x.evaluation": {"every_epochs": 1}})
    first = out["eval"][0]
    assert NEW <= set(first) and all(0.0 <= first[name] <= 1.0 for name in NEW)
