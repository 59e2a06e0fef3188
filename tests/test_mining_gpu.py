"""``PreferenceMiner`` end to end on the GPU (tiny_arch, 4 images, 4 candidates, max_length 12, threshold 0, fixed
generator): the batch it returns is what the restated rule makes of its own scores and candidates, ``DPOStep`` trains on
it, and each scorer computes what it says."""
import json
import math
import os

import numpy as np
import pytest
import torch

import mining_refs as M
from pgca_amd import REPO_ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, N, MAX_LENGTH = 4, 4, 12
S = MAX_LENGTH - 1


@pytest.fixture(scope="module")
def model():
    from pgca_amd.arch import tiny_arch
    from pgca_amd.model import PreferenceGuidedCaptioningModel
    return PreferenceGuidedCaptioningModel(freeze_vision_backbone=True, arch=tiny_arch(), seed=3, device=DEV)


@pytest.fixture(scope="module")
def images(model):
    a = model.arch.vit
    return torch.randn(B, 3, a.image, a.image, generator=torch.Generator().manual_seed(1)).to(DEV)


def gen(seed=11):
    return torch.Generator(device=DEV).manual_seed(seed)


@pytest.fixture(scope="module")
def mined(model, images):
    """One alignment-scored mining call, shared (and left unchanged) by the tests below."""
    from pgca_amd.mining import PreferenceMiner
    model.train()
    out = PreferenceMiner(model, num_candidates=N, max_length=MAX_LENGTH).mine(images, generator=gen())
    assert model.training                                   # the mode is restored
    return out


def restated_rows(model, mined):
    base = model.arch.gpt.base_vocab
    cand = mined["candidates"].cpu().numpy().reshape(B * N, S)
    return M.candidate_rows(cand, mined["lengths"].cpu().numpy().reshape(-1), S, base, model.arch.dec_vocab, base, base)


def test_the_batch_is_the_restated_rule_on_the_miners_own_scores(model, images, mined):
    rows = restated_rows(model, mined)
    base = model.arch.gpt.base_vocab
    scores = mined["scores"].cpu().numpy()
    assert scores.shape == (B, N) and np.isfinite(scores).all()
    ok = (rows["text_len"] >= 0).reshape(B, N)
    rank, pw, pl, pm, cnt = M.mine_pairs(scores, rows["dec_ids"], rows["out_len"], ok, 2, "adjacent", 0.0)
    want = M.pair_rows(pw, pl, pm, cnt, rows["dec_ids"], rows["dec_mask"], B * (N - 1), base)
    k = want["n_pairs"]
    assert mined["n_pairs"] == k and k >= 1
    assert np.array_equal(mined["rank"].cpu().numpy(), rank)
    for key in ("preferred_ids", "preferred_mask", "rejected_ids", "rejected_mask", "pair_image", "preference_score"):
        got = mined[key].cpu().numpy()
        assert got.dtype == want[key].dtype and np.array_equal(got, want[key][:k]), key
    assert torch.equal(mined["image"], images[mined["pair_image"].long()])
    assert (mined["preference_score"] >= 0).all()
    # every pair: the preferred caption outscores the rejected one of the same image, by the margin
    s = torch.from_numpy(scores)
    for r in range(k):
        b = int(mined["pair_image"][r])
        w = [j for j in range(N) if np.array_equal(rows["dec_ids"][b * N + j], want["preferred_ids"][r])][0]
        l = [j for j in range(N) if np.array_equal(rows["dec_ids"][b * N + j], want["rejected_ids"][r])][0]
        assert s[b, w] - s[b, l] == mined["preference_score"][r].cpu()


def test_the_mined_batch_trains_a_dpo_step(model, mined):
    from pgca_amd.steps import DPOStep, FusedOptimizer
    batch = {k: mined[k] for k in ("image", "preferred_ids", "preferred_mask", "rejected_ids", "rejected_mask",
                                   "preference_score")}
    # no scored row with fewer than two tokens: such a row's mean log-probability is 0/0 and the batch would be dropped
    assert int(batch["preferred_mask"].sum(1).min()) >= 2 and int(batch["rejected_mask"].sum(1).min()) >= 2
    step = DPOStep(model.store, model.ws, model.vision_encoder.tower, model.vision_encoder.head,
                   model.caption_decoder.engine, beta=0.1, reference_free=True)
    opt = FusedOptimizer([model.store.segments["vision_head"], model.store.segments["decoder"]], lr=1e-4, total_steps=4)
    p = DPOStep.prepare(batch, model.device)
    opt.zero_grad()
    loss = float(step.loss_and_grads(p["image"], p["seq"]))
    assert math.isfinite(loss)
    grad = model.store.segments["decoder"].grad
    assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0.0
    opt.zero_grad()


def test_alignment_scores_are_the_public_surface(model, images, mined):
    """The cosine of ``model(..., mode="contrastive")`` on the repeated images and the scorer rows, row-wise dot product in
    float64.  The bound is the surface's own sensitivity to batch composition, measured by tools/mining_probe.py."""
    with open(os.path.join(REPO_ROOT, "profiles", "mining.json"), "r", encoding="utf-8") as f:
        agreement = json.load(f)["score_agreement"]
    bound = float(agreement["bound"])
    P = model.arch.proj_dim
    assert bound == (4 * agreement["surface_batch_composition_max_abs_diff"] or 4 * P * 2.0 ** -24)
    rows = restated_rows(model, mined)
    model.eval()
    with torch.no_grad():
        out = model(images.repeat_interleave(N, dim=0), torch.from_numpy(rows["text_ids"]).to(DEV),
                    torch.from_numpy(rows["text_mask"]).to(DEV), mode="contrastive")
    model.train()
    want = (out["image_embeddings"].double() * out["text_embeddings"].double()).sum(1).cpu()
    err = float((mined["scores"].view(-1).double().cpu() - want).abs().max())
    print(f"alignment score vs surface: max |diff| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_logprob_scorer_is_the_length_normalised_logprob(model, images):
    from pgca_amd.mining import PreferenceMiner
    out = PreferenceMiner(model, num_candidates=N, max_length=MAX_LENGTH, scorer="logprob").mine(images, generator=gen(5))
    ids, logp, lengths = model.generate_candidates(images, N, max_length=MAX_LENGTH, generator=gen(5))
    assert torch.equal(out["candidates"][:, :, :ids.shape[2]], ids) and torch.equal(out["lengths"], lengths)
    assert torch.equal(out["scores"], logp / lengths.to(torch.float32))


def test_a_callable_scorer_decides(model, images):
    from pgca_amd.mining import PreferenceMiner
    table = torch.tensor([[0.5, 0.25, 1.0, -1.0], [0.0, 0.0, 0.0, 0.0], [3.0, 2.0, 1.0, 0.5], [-0.5, 0.75, 0.25, 2.0]],
                         device=DEV)
    seen = {}

    def scorer(imgs, dec_ids, dec_mask):
        seen.update(images=imgs, ids=dec_ids, mask=dec_mask)
        return table

    out = PreferenceMiner(model, num_candidates=N, max_length=MAX_LENGTH, scorer=scorer, rule="best_worst",
                          threshold=0.5).mine(images, generator=gen(7))
    assert torch.equal(out["scores"], table)
    assert seen["ids"].shape == seen["mask"].shape == (B, N, S) and torch.equal(seen["images"], images)
    assert torch.equal(seen["mask"].sum(2).to(torch.int32), out["out_len"])
    rows = restated_rows(model, out)
    ok = (rows["text_len"] >= 0).reshape(B, N)
    rank, pw, pl, pm, cnt = M.mine_pairs(table.cpu().numpy(), rows["dec_ids"], rows["out_len"], ok, 2, "best_worst", 0.5)
    assert np.array_equal(out["rank"].cpu().numpy(), rank) and out["n_pairs"] == int(cnt.sum())
    assert np.array_equal(out["pair_count"].cpu().numpy(), cnt) and (cnt <= 1).all()


def test_mined_data_serves_stage2_batches(model, images, mined):
    from pgca_amd.mining import MinedPreferenceData
    data = MinedPreferenceData()
    data.add(mined)
    data.add(mined)
    k = mined["n_pairs"]
    assert len(data) == 2 * k and data.stats["images"] == 2 * B and data.stats["candidates"] == 2 * B * N
    loader = data.loader(2, shuffle=False, drop_last=True)
    batches = list(loader)
    assert len(loader) == len(batches) == (2 * k) // 2
    rows = torch.cat([b["preferred_ids"] for b in batches])
    assert torch.equal(rows[:k], mined["preferred_ids"].cpu())
    assert torch.equal(torch.cat([b["image"] for b in batches])[:k], mined["image"].cpu())
    assert set(batches[0]) == {"image", "preferred_ids", "preferred_mask", "rejected_ids", "rejected_mask",
                               "preference_score"}
    shuffled = data.loader(2, shuffle=True, seed=3, drop_last=True, max_batches=1)
    assert len(shuffled) == len(list(shuffled)) == 1


def test_mine_preferences_is_the_model_surface(model, images, mined):
    out = model.mine_preferences(images, generator=gen(), num_candidates=N, max_length=MAX_LENGTH)
    assert out["n_pairs"] == mined["n_pairs"] and torch.equal(out["preferred_ids"], mined["preferred_ids"])
    assert torch.equal(out["scores"], mined["scores"])
