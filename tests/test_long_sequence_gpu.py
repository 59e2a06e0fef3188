"""Training past 512 tokens, end to end: the GPT-2 decoder at S = 640 and S = 1024 (its 1024 learned positions) and the
ViT-L/14@336 tower (577 tokens), whose attention backward runs on the split kernels (``pgca_attention_bwd_split``).

Tolerances (SURVEY 8d, bf16 MFMA operands / f32 accumulate), as in tests/test_e2e_gpu.py and tests/test_vit_train_gpu.py:
per-token log-prob |d| <= 2e-2, loss |d| <= 5e-3, gradient cosine >= 0.99, against the CPU restatement on identical
weights and batch."""
import functools

import pytest
import torch

from oracle import restatement as R

pytestmark = pytest.mark.gpu
DEC = "caption_decoder.lm_model.transformer."
VM = "vision_encoder.vision_model."


def cos(a, b):
    a, b = a.double().flatten().cpu(), torch.as_tensor(b).double().flatten()
    return float((a @ b) / (a.norm() * b.norm() + 1e-30))


def _arch():
    from pgca_amd.arch import VIT_ZOO, GptArch, ModelArch
    return ModelArch(vit=VIT_ZOO["tiny-vit"], gpt=GptArch(128, 2, 2, n_pos=1024, base_vocab=509), proj_dim=64)


def _batch(S, lens):
    arch = _arch()
    gen = torch.Generator().manual_seed(1000 + S)
    B = len(lens) // 2
    ids = torch.randint(0, arch.gpt.base_vocab, (2 * B, S), generator=gen)
    mask = (torch.arange(S)[None] < torch.tensor(lens)[:, None]).long()
    ids = torch.where(mask.bool(), ids, torch.full_like(ids, arch.gpt.base_vocab))
    img = torch.randn(B, 3, arch.vit.image, arch.vit.image, generator=gen)
    return img, ids, mask


@functools.lru_cache(maxsize=None)
def _dpo_step(S, lens, mode, run=0):
    """One Stage-2 4-forward DPO step (packed rows, eval mode) of the tiny geometry with 1024 positions; the reference
    policy is the snapshot with every block's mlp.c_proj scaled by 0.9, as in the tiny end-to-end fixture.  ``run`` only
    tells two otherwise identical runs apart."""
    from pgca_amd.model import PreferenceGuidedCaptioningModel
    from pgca_amd.steps import DPOStep, ReferencePolicy
    arch = _arch()
    model = PreferenceGuidedCaptioningModel(freeze_vision_backbone=True, arch=arch, seed=3, device="cuda:0")
    ref = ReferencePolicy(model.store, model.ws)
    seg = ref.store.segments["decoder"]
    for name in seg.index:
        if ".h." in name and name.endswith("mlp.c_proj.weight"):
            seg.w(name).mul_(0.9)
    seg.ensure_bf16()
    img, ids, mask = _batch(S, lens)
    B = img.shape[0]
    batch = {"image": img, "preferred_ids": ids[:B], "rejected_ids": ids[B:], "preferred_mask": mask[:B],
             "rejected_mask": mask[B:]}
    step = DPOStep(model.store, model.ws, model.vision_encoder.tower, model.vision_encoder.head,
                   model.caption_decoder.engine, beta=0.1, reference_free=False, ref=ref, packed=True, recompute=mode)
    p = DPOStep.prepare(batch, model.device)
    assert p["seq"].pack is not None
    for s in model.store.trainable_segments():
        s.grad.zero_()
    loss = float(step.loss_and_grads(p["image"], p["seq"]))
    torch.cuda.synchronize()
    pol = model.ws.bufs["pol.seq_lp"][:2 * B].cpu().clone()
    grads = {name: seg.g(name).clone() for seg in model.store.trainable_segments() for name in seg.index}
    sd = {k: v.detach().cpu().clone() for k, v in model.store.state_dict(aliases=False).items()}
    sd_ref = {k: v.detach().cpu().clone() for k, v in ref.store.state_dict(aliases=False).items()}
    return loss, pol, grads, sd, sd_ref


@pytest.mark.parametrize("S,lens", [(640, (640, 513, 37, 513, 640, 37)), (1024, (1024, 513, 37, 897, 1024, 130))],
                         ids=["S640", "S1024"])
def test_long_sequence_dpo_step_against_oracle(S, lens):
    arch = _arch()
    loss, pol, grads, sd, sd_ref = _dpo_step(S, lens, "none")
    img, ids, mask = _batch(S, lens)
    B = img.shape[0]
    sd = {k: v.clone().requires_grad_(k.startswith(("caption_decoder", "vision_encoder.projection")))
          for k, v in sd.items()}
    full_ref = {**{k: v.detach() for k, v in sd.items()}, **sd_ref}

    def seq_lp(weights, rows):
        logits = R.model_forward(weights, img, ids[rows], mask[rows], "generation", arch.vit.heads, arch.vit.patch,
                                 arch.gpt.heads)["logits"]
        return R.sequence_logprob_sum(logits, ids[rows], mask[rows])

    w, l = slice(0, B), slice(B, 2 * B)
    pw, pl = seq_lp(sd, w), seq_lp(sd, l)
    with torch.no_grad():
        rw, rl = seq_lp(full_ref, w), seq_lp(full_ref, l)
    ref_loss, _ = R.dpo_loss(pw, pl, rw, rl, beta=0.1)
    ref_loss.backward()
    scored = mask[:, 1:].sum(-1).double()
    per_token = ((pol.double() - torch.cat([pw, pl]).detach().double()).abs() / scored)
    print(f"S={S}: per-token log-prob |d| {per_token.tolist()}, loss {loss:.6f} vs {float(ref_loss):.6f}")
    assert float(per_token.max()) <= 2e-2
    assert abs(loss - float(ref_loss)) <= 5e-3, (loss, float(ref_loss))
    names = [DEC + "wte.weight", DEC + "wpe.weight"]
    for i in (0, 1):
        names += [DEC + f"h.{i}.attn.c_attn.weight", DEC + f"h.{i}.attn.c_proj.weight", DEC + f"h.{i}.mlp.c_fc.weight",
                  DEC + f"h.{i}.mlp.c_proj.weight"]
    names += ["caption_decoder.vision_projection.0.weight", "caption_decoder.cross_attention.out_proj.weight",
              "caption_decoder.attention_norm.weight", "vision_encoder.projection.0.weight",
              "vision_encoder.projection.4.weight"]
    for name in names:
        c = cos(grads[name], sd[name].grad)
        print(f"S={S} {name}: cosine {c:.6f}")
        assert c >= 0.99, f"{name}: cosine {c}"


# Gradients that sit behind a float atomic of the embedding backward (csrc/layernorm.hip: embed_bwd_kernel adds into wte
# and into the per-sequence gradient of the attended vector with atomicAdd), so that two runs of the SAME mode differ.
# Measured at this S = 640 step, 8 runs of mode none, 28 pairs, max |difference| over the tensor's max |gradient|:
#   f32 sums of the atomics themselves: every pair differs, by <= 6.7e-8 (wte) and <= 3.8e-7 (cross-attention out bias);
#   the head path behind them: the attended-vector gradient is cast to bf16 for its GEMMs, and an order difference of
#   ~4e-8 moves an element to the neighbouring bf16 value in some runs - 12 of 28 pairs differ, by 8.4e-4 ... 3.9e-3
#   (largest: vision_encoder.projection.0), the other 16 pairs are bit-equal.
# So bit equality cannot be asked of these between ANY two runs, and the project's rule (tests/test_recompute_gpu.py:
# equal wherever two runs of none are equal) fails by chance here: two none runs agree in 16 of 28 cases and the third
# run then differs.  They are held to twice the measured none-vs-none maximum of their class instead; everything else -
# every block parameter, ln_f, wpe, attention_norm - must be torch.equal.
_F32_ATOMIC = (DEC + "wte.weight", "caption_decoder.cross_attention.out_proj.bias")
_BF16_BEHIND_ATOMIC = ("vision_encoder.projection.", "caption_decoder.vision_projection.",
                       "caption_decoder.cross_attention.in_proj_", "caption_decoder.cross_attention.out_proj.weight")
_F32_ATOMIC_BOUND = 2 * 3.8e-7
_BF16_BEHIND_ATOMIC_BOUND = 2 * 3.9e-3


@pytest.mark.parametrize("mode", ["mlp", "block"])
def test_long_sequence_recompute_is_bit_identical(mode):
    """The S = 640 step under a recompute mode against mode none: the backward rebuilds what the forward did not keep
    with the same kernels on the same inputs, so the gradients are the same bits - except behind the float atomics
    described above, where two runs of none differ as well."""
    S, lens = 640, (640, 513, 37, 513, 640, 37)
    loss_a, _, ga, _, _ = _dpo_step(S, lens, "none")
    loss_n, _, gn, _, _ = _dpo_step(S, lens, "none", run=1)
    loss_m, _, gm, _, _ = _dpo_step(S, lens, mode)
    assert loss_a == loss_n == loss_m
    exact = [n for n in ga if n not in _F32_ATOMIC and not n.startswith(_BF16_BEHIND_ATOMIC)]
    assert sum(".h." in n for n in exact) >= 2 * 12 and DEC + "wpe.weight" in exact
    assert any(".h." in n and float(ga[n].abs().max()) > 0 for n in exact)
    for name in ga:
        scale = float(ga[name].abs().max())
        d, dn = (float((g[name] - ga[name]).abs().max()) for g in (gm, gn))
        if name in exact:
            assert torch.equal(gn[name], ga[name]), f"{name}: two runs of none differ by {dn}"
            assert torch.equal(gm[name], ga[name]), f"{mode}: {name} differs by {d}"
            continue
        bound = _F32_ATOMIC_BOUND if name in _F32_ATOMIC else _BF16_BEHIND_ATOMIC_BOUND
        print(f"{mode} {name}: |diff| / max {d / scale:.3e}, none-vs-none {dn / scale:.3e}, bound {bound:.1e}")
        assert d <= bound * scale, f"{mode}: {name} differs by {d / scale:.3e} of its maximum (bound {bound:.1e})"


def test_vit_l14_336_trainable_tower_against_oracle():
    """openai/clip-vit-large-patch14-336 at real width (1024 wide, 16 heads, 24 x 24 + 1 = 577 tokens over five 128-row
    blocks, patch K = 588 padded to 640), 2 layers, B = 2: the recipe of
    tests/test_vit_train_gpu.py::test_real_width_tower_backward_against_oracle."""
    from pgca_amd.arch import make_arch, with_layers
    from pgca_amd.model import PreferenceGuidedCaptioningModel
    from pgca_amd.steps import ContrastiveStep
    arch = with_layers(make_arch("openai/clip-vit-large-patch14-336", "gpt2", 512), 2, 1)
    assert arch.vit.tokens == 577 and arch.vit.grid == 24
    model = PreferenceGuidedCaptioningModel(arch=arch, seed=29, device="cuda:0")
    vit = model.store.segments["vit"]
    for name in vit.index:
        if name.endswith(("self_attn.v_proj.weight", "self_attn.out_proj.weight")):
            vit.w(name).mul_(4.0)
    vit.ensure_bf16()
    gen = torch.Generator().manual_seed(78)
    B, S = 2, 32
    img = torch.randn(B, 3, arch.vit.image, arch.vit.image, generator=gen)
    ids = torch.randint(0, 50257, (B, S), generator=gen)
    mask = (torch.arange(S)[None] < torch.tensor([32, 9])[:, None]).long()
    ids = torch.where(mask.bool(), ids, torch.full_like(ids, 50257))
    sd = {k: v.detach().cpu().clone().requires_grad_(k.startswith("vision_encoder"))
          for k, v in model.store.state_dict(aliases=False).items()}
    ref_vis = R.vision_encoder_forward(sd, img, arch.vit.heads, arch.vit.patch)
    # the forward that keeps nothing (what a frozen tower runs)
    vis = model.vision_encoder(img)
    assert vis["features"].shape == (B, 577, 1024)
    assert cos(vis["features"], ref_vis["features"].detach()) >= 0.999
    step = ContrastiveStep(model.store, model.ws, model.vision_encoder.tower, model.vision_encoder.head,
                           model.text_encoder.engine, temperature=0.5)
    p = ContrastiveStep.prepare({"image": img, "caption_ids": ids, "caption_mask": mask}, model.device)
    for s in model.store.trainable_segments():
        s.grad.zero_()
    loss = float(step.loss_and_grads(p["image"], p["ids"], p["mask"]))
    with torch.no_grad():
        te = R.text_encoder_forward(sd, ids, mask, arch.gpt.heads)["embeddings"]
    ref = R.nt_xent(torch.nn.functional.normalize(ref_vis["embeddings"], dim=-1),
                    torch.nn.functional.normalize(te, dim=-1), 0.5)
    ref.backward()
    print(f"loss {loss:.6f} vs {float(ref):.6f}")
    assert abs(loss - float(ref)) <= 5e-3, (loss, float(ref))
    for name in ("embeddings.class_embedding", "embeddings.patch_embedding.weight", "embeddings.position_embedding.weight",
                 "pre_layrnorm.weight", "pre_layrnorm.bias", "post_layernorm.weight", "post_layernorm.bias",
                 "encoder.layers.0.self_attn.q_proj.weight", "encoder.layers.0.self_attn.k_proj.weight",
                 "encoder.layers.0.self_attn.v_proj.weight", "encoder.layers.0.self_attn.v_proj.bias",
                 "encoder.layers.1.self_attn.out_proj.weight", "encoder.layers.1.self_attn.out_proj.bias",
                 "encoder.layers.0.layer_norm1.weight", "encoder.layers.1.layer_norm2.bias",
                 "encoder.layers.0.mlp.fc1.weight", "encoder.layers.1.mlp.fc1.bias", "encoder.layers.0.mlp.fc2.weight",
                 "encoder.layers.1.mlp.fc2.bias"):
        c = cos(model.store.g(VM + name), sd[VM + name].grad)
        print(f"{name}: cosine {c:.6f}")
        assert c >= 0.99, f"{name}: cosine {c}"
    assert cos(model.store.g("vision_encoder.projection.0.weight"), sd["vision_encoder.projection.0.weight"].grad) >= 0.99
