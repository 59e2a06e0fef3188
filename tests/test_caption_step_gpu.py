"""``steps.CaptionStep`` (the decoder's language-model loss), ``steps.DPOStep(sft_alpha=...)`` and the ``labels=`` surface
with HF's ignore index, on the tiny model of ``tests/golden/tiny_e2e.npz`` (built as ``test_e2e_gpu.py`` builds it).

Oracle: ``oracle.restatement`` on the host with the masked cross-entropy of ``caption_refs.masked_ce`` and autograd, and
the reference's own logits in the fixture.  Tolerances are the project's (as in ``test_e2e_gpu.py``): loss
|d| <= 5e-3, gradient cosine >= 0.99; against the reference's stored logits 2e-2 (the constant of the existing surface
test for this quantity); packed against padded as ``test_packed_gpu.py``: loss <= 1e-6, cosine >= 0.99999.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import caption_refs as C
from oracle import restatement as R

pytestmark = pytest.mark.gpu
T = torch.from_numpy
cos = C.cos
DEC = "caption_decoder.lm_model.transformer."
WTE = DEC + "wte.weight"


@pytest.fixture(scope="module")
def tiny(golden):
    from pgca_amd.arch import tiny_arch
    from pgca_amd.model import PreferenceGuidedCaptioningModel
    g = golden("tiny_e2e")
    model = PreferenceGuidedCaptioningModel(freeze_vision_backbone=True, arch=tiny_arch(), seed=int(g["seed"]),
                                            device="cuda:0")
    for seg in model.store.segments.values():
        chk = g[f"chk_{seg.name}"]
        assert abs(float(seg.fp32.double().sum()) - chk[0]) <= 1e-5 * max(1.0, abs(chk[0]))
    return g, model


def host_weights(model):
    return {k: v.detach().cpu().clone().requires_grad_(not k.startswith("vision_encoder.vision_model"))
            for k, v in model.store.state_dict(aliases=False).items()}


def oracle_logits(sd, arch, img, ids, mask, drop=None):
    emb = R.vision_encoder_forward(sd, img, arch.vit.heads, arch.vit.patch, drop)["embeddings"]
    return R.caption_decoder_logits(sd, emb, ids, mask, arch.gpt.heads, drop)


def oracle_grads(sd, loss):
    names = [k for k, v in sd.items() if v.requires_grad]
    grads = torch.autograd.grad(loss, [sd[k] for k in names], allow_unused=True)
    return {k: gr.detach().clone() for k, gr in zip(names, grads) if gr is not None}


@pytest.fixture(scope="module")
def oracle(tiny):
    """Computed once, shared and left unchanged: the oracle's loss and gradients on (images, ids_w, mask_w)."""
    g, model = tiny
    sd = host_weights(model)
    img, ids, mask = T(g["images"]), T(g["ids_w"]), T(g["mask_w"])
    logits = oracle_logits(sd, model.arch, img, ids, mask)
    loss = C.masked_ce(logits, ids, mask)
    return {"loss": float(loss), "grads": oracle_grads(sd, loss), "logits": logits.detach()}


def caption_step(model, **kw):
    from pgca_amd.steps import CaptionStep
    return CaptionStep(model.store, model.ws, model.vision_encoder.tower, model.vision_encoder.head,
                       model.caption_decoder.engine, **kw)


def dpo_step(model, reference_free, ref=None, **kw):
    from pgca_amd.steps import DPOStep
    return DPOStep(model.store, model.ws, model.vision_encoder.tower, model.vision_encoder.head,
                   model.caption_decoder.engine, beta=0.1, reference_free=reference_free, ref=ref, **kw)


def caption_batch(model, img, ids, mask):
    from pgca_amd.steps import CaptionStep
    return CaptionStep.prepare({"image": img, "caption_ids": ids, "caption_mask": mask}, model.device)


def pair_batch(g, model):
    from pgca_amd.steps import DPOStep
    return DPOStep.prepare({"image": T(g["images"]), "preferred_ids": T(g["ids_w"]), "rejected_ids": T(g["ids_l"]),
                            "preferred_mask": T(g["mask_w"]), "rejected_mask": T(g["mask_l"])}, model.device)


def zero_grads(model):
    for s in model.store.trainable_segments():
        s.grad.zero_()


def grads_of(model):
    out = {}
    for seg in model.store.trainable_segments():
        for name in seg.index:
            out[name] = seg.g(name).clone()
    return out


def bitwise_class(name):
    """Gradients with no float atomic on their way, bitwise reproducible from run to run (as test_long_sequence_gpu.py
    holds them): block parameters, ln_f, wpe, attention_norm.  The rest - wte and what the embedding backward's atomic
    sum of the attended-vector gradient feeds: the cross-attention / vision_projection prefix and the vision head -
    may differ in the order of their sums."""
    return (".h." in name or ".ln_f." in name or name.endswith(".wpe.weight")
            or name.startswith("caption_decoder.attention_norm."))


def checked_names(g, ref_grads):
    """The tensors the DPO tests check (the fixture's ``s2_grad::`` names), wte and the vision head."""
    names = [k[len("s2_grad::"):] for k in g.files if k.startswith("s2_grad::")] + [WTE]
    names += [k for k in ref_grads if k.startswith("vision_encoder.projection")]
    return [n for n in dict.fromkeys(names) if n in ref_grads]


def assert_grads_match(model, g, ref_grads, what):
    names = checked_names(g, ref_grads)
    assert WTE in names and any(n.startswith("vision_encoder.projection") for n in names) and len(names) > 6
    for name in names:
        got, want = model.store.g(name), ref_grads[name]
        if float(want.abs().max()) == 0:
            assert float(got.abs().max()) == 0.0, f"{what} {name}"
        else:
            c = cos(got, want)
            assert c >= 0.99, f"{what} {name}: cosine {c}"


# ------------------------------------------------------------------------------------------------ loss and gradients
def test_loss_and_gradients_match_the_oracle(tiny, oracle):
    g, model = tiny
    step = caption_step(model)
    p = caption_batch(model, T(g["images"]), T(g["ids_w"]), T(g["mask_w"]))
    zero_grads(model)
    loss = float(step.loss_and_grads(p["image"], p["seq"]))
    ref_logits = T(g["s2_logits_w"]).double()                 # the reference's own logits
    ref_loss = float(C.masked_ce(ref_logits, T(g["ids_w"]), T(g["mask_w"])))
    print(f"caption loss {loss:.6f}  oracle {oracle['loss']:.6f}  reference logits {ref_loss:.6f}")
    assert abs(loss - oracle["loss"]) <= 5e-3
    assert abs(loss - ref_loss) <= 2e-2
    met = step.metrics.cpu()
    assert float(met[1]) == float((T(g["mask_w"])[:, 1:] != 0).sum()) and float(met[3]) == 1.0 and float(met[2]) == loss
    assert abs(float(step.loss_only(p["image"], p["seq"])) - loss) <= 1e-6
    assert_grads_match(model, g, oracle["grads"], "caption")
    # q/k rows of the collapsed cross-attention receive exactly zero (not missing) gradient
    H = model.arch.gpt.hidden
    gi = model.store.g("caption_decoder.cross_attention.in_proj_weight")
    assert float(gi[:2 * H].abs().max()) == 0.0 and float(gi[2 * H:].abs().max()) > 0
    # nothing reaches the text tower
    assert float(model.store.segments["text_tower"].grad.abs().max()) == 0.0
    for name in ("text_tower", "text_head"):
        assert float(model.store.segments[name].grad.abs().max()) == 0.0


def test_prepare_reads_the_chosen_side_of_a_preference_batch(tiny):
    from pgca_amd.steps import CaptionStep
    g, model = tiny
    b = {"image": T(g["images"]), "preferred_ids": T(g["ids_w"]), "rejected_ids": T(g["ids_l"]),
         "preferred_mask": T(g["mask_w"]), "rejected_mask": T(g["mask_l"])}
    p = CaptionStep.prepare(b, model.device)
    q = caption_batch(model, T(g["images"]), T(g["ids_w"]), T(g["mask_w"]))
    assert p["seq"].Bq == 4 and torch.equal(p["seq"].targets, q["seq"].targets)
    assert torch.equal(p["seq"].row_map, q["seq"].row_map)
    # caption_* wins when both are there
    b.update(caption_ids=T(g["ids_l"]), caption_mask=T(g["mask_l"]))
    r = CaptionStep.prepare(b, model.device)
    assert torch.equal(r["seq"].ids.cpu(), T(g["ids_l"]))


def test_ragged_masks_with_a_one_token_caption(tiny):
    g, model = tiny
    img, ids = T(g["images"]), T(g["ids_w"])
    S = ids.shape[1]
    mask = (torch.arange(S)[None] < torch.tensor([S, 1, 5, 9])[:, None]).long()
    p = caption_batch(model, img, ids, mask)
    assert p["seq"].counts.cpu().tolist() == [S - 1, 0, 4, 8] and p["seq"].n_rows == S + 11
    step = caption_step(model)
    zero_grads(model)
    loss = float(step.loss_and_grads(p["image"], p["seq"]))
    sd = host_weights(model)
    ref = C.masked_ce(oracle_logits(sd, model.arch, img, ids, mask), ids, mask)
    assert math.isfinite(loss) and abs(loss - float(ref)) <= 5e-3
    assert_grads_match(model, g, oracle_grads(sd, ref), "ragged")
    # the caption that scores nothing contributes nothing: the token count of the mean is the other three captions', and
    # loss and gradients are those of the batch WITHOUT it (bounds of the packed-against-padded comparison: the same
    # rows through the same kernels, up to the order of the embedding tables' atomic sums)
    assert float(step.metrics[1]) == float(S - 1 + 4 + 8) == float((mask[:, 1:] != 0).sum())
    with_it = grads_of(model)
    rest = torch.tensor([0, 2, 3])
    q = caption_batch(model, img[rest], ids[rest], mask[rest])
    zero_grads(model)
    loss_rest = float(step.loss_and_grads(q["image"], q["seq"]))
    assert abs(loss - loss_rest) <= 1e-6 and float(step.metrics[1]) == float(S + 11)
    for name, a in grads_of(model).items():
        if float(a.abs().max()) == 0:
            assert float(with_it[name].abs().max()) == 0.0, name
        else:
            assert cos(with_it[name], a) >= 0.99999, f"{name}: cosine {cos(with_it[name], a)}"
    # the step only refuses a batch in which NO token is scored
    with pytest.raises(ValueError, match="no scored token"):
        caption_batch(model, img, ids, (torch.arange(S)[None] < torch.ones(4, 1)).long())


def test_packed_against_padded(tiny):
    g, model = tiny
    p = caption_batch(model, T(g["images"]), T(g["ids_w"]), T(g["mask_w"]))
    out = {}
    for packed in (True, False):
        step = caption_step(model, packed=packed)
        zero_grads(model)
        out[packed] = (float(step.loss_and_grads(p["image"], p["seq"])), grads_of(model))
    assert abs(out[True][0] - out[False][0]) <= 1e-6
    for name, a in out[True][1].items():
        b = out[False][1][name]
        if float(b.abs().max()) == 0:
            assert float(a.abs().max()) == 0.0, name
        else:
            assert cos(a, b) >= 0.99999, f"{name}: cosine {cos(a, b)}"


def test_accumulation_of_two_micro_batches(tiny):
    """Two micro-batches at loss_scale = 0.5 sum to the gradient of the mean of the two losses."""
    g, model = tiny
    img, ids, mask = T(g["images"]), T(g["ids_w"]), T(g["mask_w"])
    step = caption_step(model)
    zero_grads(model)
    losses = []
    for sl in (slice(0, 2), slice(2, 4)):
        p = caption_batch(model, img[sl], ids[sl], mask[sl])
        losses.append(float(step.loss_and_grads(p["image"], p["seq"], loss_scale=0.5)))
    sd = host_weights(model)
    refs = [C.masked_ce(oracle_logits(sd, model.arch, img[sl], ids[sl], mask[sl]), ids[sl], mask[sl])
            for sl in (slice(0, 2), slice(2, 4))]
    for got, want in zip(losses, refs):                       # the returned loss is the unscaled one
        assert abs(got - float(want)) <= 5e-3
    assert_grads_match(model, g, oracle_grads(sd, 0.5 * (refs[0] + refs[1])), "accumulated")


def test_train_mode_dropout_matches_the_oracle_with_the_same_masks(tiny):
    from pgca_amd.engine import DropoutPlan
    g, model = tiny
    img, ids, mask = T(g["images"]), T(g["ids_w"]), T(g["mask_w"])
    seed, p_drop = 4242, 0.1
    plan = DropoutPlan(p_drop, seed)
    plan.step = 3
    step = caption_step(model, dropout=plan)
    p = caption_batch(model, img, ids, mask)
    zero_grads(model)
    loss = float(step.loss_and_grads(p["image"], p["seq"]))
    assert plan.step == 4
    sd = host_weights(model)
    ref = C.masked_ce(oracle_logits(sd, model.arch, img, ids, mask, R.Dropper(seed, p_drop, step=3)), ids, mask)
    assert abs(loss - float(ref)) <= 5e-3
    assert abs(float(step.loss_only(p["image"], p["seq"])) - loss) > 1e-4      # the masks really were applied
    assert_grads_match(model, g, oracle_grads(sd, ref), "train mode")


def test_recompute_modes_are_bitwise_none(tiny):
    """``mlp`` / ``block`` against ``none``: block parameters, ln_f, wpe and attention_norm are ``torch.equal``, between
    two runs of ``none`` too (``bitwise_class``); the classes behind a float atomic (wte, the cross-attention prefix
    path and the vision head behind it) are bitwise when two runs of ``none`` are, else within 4 x their spread."""
    from pgca_amd.engine import DropoutPlan
    g, model = tiny
    p = caption_batch(model, T(g["images"]), T(g["ids_w"]), T(g["mask_w"]))

    def run(mode):
        step = caption_step(model, dropout=DropoutPlan(0.1, base_seed=5), recompute=mode)
        assert model.caption_decoder.engine.trunk.recompute == mode
        zero_grads(model)
        loss = step.loss_and_grads(p["image"], p["seq"]).clone()
        return loss, grads_of(model)

    try:
        loss_a, ga = run("none")
        loss_b, gb = run("none")
        assert torch.equal(loss_a, loss_b) and bool(torch.isfinite(loss_a).all())
        spread = {n: float((ga[n] - gb[n]).abs().max()) for n in ga}
        for n, d in spread.items():
            assert d == 0.0 or not bitwise_class(n), f"{n}: two runs of none differ by {d}"
        held = [n for n in ga if n.startswith("caption_decoder") and bitwise_class(n) and ".h." not in n]
        assert len(held) == 5 and all(float(ga[n].abs().max()) > 0 for n in held)   # ln_f w/b, wpe, attention_norm w/b
        assert any(".h." in n and float(ga[n].abs().max()) > 0 for n in ga)
        for mode in ("mlp", "block"):
            loss_m, gm = run(mode)
            assert torch.equal(loss_m, loss_a), mode
            for n in ga:
                if spread[n] == 0.0 or bitwise_class(n):
                    assert torch.equal(gm[n], ga[n]), f"{mode}: {n}"
                else:
                    assert float((gm[n] - ga[n]).abs().max()) <= 4 * spread[n], f"{mode}: {n}"
    finally:
        model.caption_decoder.engine.trunk.recompute = "none"


def test_nan_in_a_decoder_bias_adds_no_gradient(tiny, oracle):
    """A NaN in ``ln_f.bias`` makes every token log-prob NaN: the loss is not finite and the step must leave every
    gradient buffer exactly zero.

    Zero seeds alone do not do that: the NaN activations the forward saved turn them into NaN in the DLOGITS epilogue
    and in every weight-gradient GEMM (measured with the backward launched: 505984 NaN elements in this decoder's
    gradient buffer, 8545 in the vision head's).  The step reads the finite flag back and does not launch the backward;
    the trunk's per-layer gradient hook - a data-parallel reducer's collectives - must still fire as in a real
    backward, and the next step must find nothing left over."""
    g, model = tiny
    seg = model.store.seg_of(DEC + "ln_f.bias")
    bias = seg.w(DEC + "ln_f.bias")
    keep = bias.clone()
    p = caption_batch(model, T(g["images"]), T(g["ids_w"]), T(g["mask_w"]))
    step = caption_step(model)
    trunk = model.caption_decoder.engine.trunk
    fired = []
    try:
        trunk.grad_hook = fired.append
        zero_grads(model)
        step.loss_and_grads(p["image"], p["seq"])
        torch.cuda.synchronize()
        real, fired[:] = list(fired), []
        assert sorted(real, reverse=True) == real == list(range(model.arch.gpt.layers - 1, -1, -1))
        bias[3] = float("nan")
        seg.ensure_bf16()
        zero_grads(model)
        loss = float(step.loss_and_grads(p["image"], p["seq"]))
        torch.cuda.synchronize()
        dirty = {s.name: int((s.grad != 0).sum()) for s in model.store.trainable_segments()}
    finally:
        trunk.grad_hook = None
        bias.copy_(keep)
        seg.ensure_bf16()
        zero_grads(model)
    print(f"loss {loss}, non-zero gradient elements per segment: {dirty}")
    assert not math.isfinite(loss)
    assert float(step.metrics[3]) == 0.0
    assert all(v == 0 for v in dirty.values()), dirty
    assert fired == real                                     # the skipped backward fired the same hooks in the same order
    # the value restored: the next step is an ordinary one
    again = float(step.loss_and_grads(p["image"], p["seq"]))
    assert abs(again - oracle["loss"]) <= 5e-3
    assert_grads_match(model, g, oracle["grads"], "after a skipped micro-batch")
    zero_grads(model)


# ------------------------------------------------------------------------------------------------ DPO + NLL
def _ref_policy(model):
    """The fixture's reference policy: a snapshot with mlp.c_proj scaled by 0.9 (as test_e2e_gpu.py)."""
    from pgca_amd.steps import ReferencePolicy
    ref = ReferencePolicy(model.store, model.ws)
    seg = ref.store.segments["decoder"]
    for name in seg.index:
        if ".h." in name and name.endswith("mlp.c_proj.weight"):
            seg.w(name).mul_(0.9)
    seg.ensure_bf16()
    return ref


@pytest.mark.parametrize("reference_free", [True, False], ids=["2fwd", "4fwd"])
def test_sft_alpha_zero_is_the_step_without_the_argument(tiny, reference_free):
    g, model = tiny
    ref = None if reference_free else _ref_policy(model)
    p = pair_batch(g, model)
    out = []
    for kw in ({}, {"sft_alpha": 0.0}):
        step = dpo_step(model, reference_free, ref, **kw)
        zero_grads(model)
        loss = step.loss_and_grads(p["image"], p["seq"]).clone()
        out.append((loss, step.metrics.clone(), grads_of(model)))
    (la, ma, ga), (lb, mb, gb) = out
    assert torch.equal(la, lb) and torch.equal(ma, mb)
    for n in ga:
        if bitwise_class(n):
            assert torch.equal(ga[n], gb[n]), n
        else:
            assert cos(ga[n], gb[n]) >= 0.99999 or float(ga[n].abs().max()) == 0.0, n


@pytest.mark.parametrize("reference_free", [True, False], ids=["2fwd", "4fwd"])
def test_sft_alpha_adds_the_chosen_captions_nll(tiny, oracle, reference_free):
    g, model = tiny
    alpha, B = 0.5, 4
    ref = None if reference_free else _ref_policy(model)
    p = pair_batch(g, model)
    runs = {}
    for a in (0.0, alpha):
        step = dpo_step(model, reference_free, ref, sft_alpha=a)
        zero_grads(model)
        runs[a] = (float(step.loss_and_grads(p["image"], p["seq"])), grads_of(model), float(step.nll))
        if a:
            assert abs(float(step.loss_only(p["image"], p["seq"])) - runs[a][0]) <= 1e-6
            assert float(step.nll_metrics[1]) == float((T(g["mask_w"])[:, 1:] != 0).sum())
    want_dpo = float(g["s2_pref_loss"] if reference_free else g["s2_dpo_loss"])        # the reference's own value
    assert abs(runs[0.0][0] - want_dpo) <= 5e-3
    assert abs(runs[alpha][2] - oracle["loss"]) <= 5e-3
    assert abs(runs[alpha][0] - (want_dpo + alpha * oracle["loss"])) <= 5e-3
    # grads(alpha) - grads(0) against alpha * grads(CaptionStep on the chosen batch)
    cstep = caption_step(model)
    q = caption_batch(model, T(g["images"]), T(g["ids_w"]), T(g["mask_w"]))
    zero_grads(model)
    cstep.loss_and_grads(q["image"], q["seq"])
    gc = grads_of(model)
    checked = 0
    for n in checked_names(g, oracle["grads"]):
        want = alpha * gc[n]
        diff = runs[alpha][1][n] - runs[0.0][1][n]
        if float(want.abs().max()) == 0:
            assert float(diff.abs().max()) == 0.0, n
            continue
        c = cos(diff, want)
        assert c >= 0.99, f"{n}: cosine {c}"
        checked += 1
    assert checked > 6


def test_sft_term_non_finite_zeroes_the_micro_batch(tiny):
    """A rejected caption with one real token makes the 2-forward (length-mean) DPO term 0/0 while the chosen captions'
    NLL is finite: the returned loss is not finite and nothing is added to any gradient buffer."""
    from pgca_amd.steps import DPOStep
    g, model = tiny
    S = g["ids_w"].shape[1]
    mask_l = T(g["mask_l"]).clone()
    mask_l[1] = (torch.arange(S) < 1).long()
    p = DPOStep.prepare({"image": T(g["images"]), "preferred_ids": T(g["ids_w"]), "rejected_ids": T(g["ids_l"]),
                         "preferred_mask": T(g["mask_w"]), "rejected_mask": mask_l}, model.device)
    step = dpo_step(model, True, sft_alpha=0.5)
    zero_grads(model)
    loss = float(step.loss_and_grads(p["image"], p["seq"]))
    assert not math.isfinite(loss) and math.isfinite(float(step.nll))
    for s in model.store.trainable_segments():
        assert float(s.grad.abs().max()) == 0.0, s.name


# ------------------------------------------------------------------------------------------------ surface
def test_labels_with_the_ignore_index(tiny):
    """-100 on a prefix and on the padded positions, against F.cross_entropy(ignore_index=-100) on the reference's own
    logits; labels without -100 keep today's all-positions mean."""
    g, model = tiny
    img, ids, mask = T(g["images"]), T(g["ids_w"]), T(g["mask_w"])
    labels = torch.where(mask != 0, ids, torch.full_like(ids, -100))
    labels[:, :3] = -100
    out = model(images=img, caption_ids=ids, caption_mask=mask, labels=labels, mode="generation")
    ref_logits = T(g["s2_logits_w"]).double()
    V = ref_logits.shape[-1]
    want = F.cross_entropy(ref_logits[:, :-1].reshape(-1, V), labels[:, 1:].reshape(-1), ignore_index=-100)
    got = float(out["generation_loss"])
    print(f"generation_loss with -100: {got:.6f}, reference logits {float(want):.6f}")
    assert abs(got - float(want)) <= 2e-2
    full = model(images=img, caption_ids=ids, caption_mask=mask, labels=ids, mode="generation")
    want_full = F.cross_entropy(ref_logits[:, :-1].reshape(-1, V), ids[:, 1:].reshape(-1))
    assert abs(float(full["generation_loss"]) - float(want_full)) <= 2e-2
    assert abs(float(full["generation_loss"]) - got) > 1e-3          # the ignored positions really were left out
    # every label ignored: the mean over nothing, NaN as HF returns it (not an error)
    none = model(images=img, caption_ids=ids, caption_mask=mask, labels=torch.full_like(ids, -100), mode="generation")
    assert math.isnan(float(none["generation_loss"])) and none["logits"].shape == full["logits"].shape
