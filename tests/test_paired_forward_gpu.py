"""Paired forward of the policy and reference trunks (``CaptionDecoderEngine.sequence_logprobs_pair``): one walk over
the layers, the four GEMMs of a layer launched once for both trunks.

A whole ``DPOStep.loss_and_grads`` with the paired path against the same step with ``gemm_group = 0`` (every GEMM on its
own): loss, both sets of sequence log-probs and every saved activation must be BITWISE equal - the paired launch runs
the separate launches' tiles.  The backward then starts from identical inputs, so gradients differ only where two runs
of the unpaired path differ from each other: the f32 atomics behind the LM head / embedding gradients.  That spread is
measured here (two unpaired runs) and is the bound, with the f32 rounding of a reordered sum as its floor; block and
ln_f gradients have no atomics on their path and must agree bit for bit.

Geometry: the tiny config of ``test_e2e_gpu`` (hidden 128, 2 layers), ragged lengths on packed rows, train-mode dropout.
The 256^2 tile is forced - at 128 packed rows the library would pick the 128^2 kernel, which is never paired.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

LENS = [32, 9, 20, 5, 17, 31]
S = 32


@pytest.fixture(scope="module", autouse=True)
def tile256():
    from pgca_amd import hip
    hip.load()
    hip.set_option("gemm_tile", 256)
    yield
    hip.set_option("gemm_tile", 0)
    hip.set_option("gemm_group", 1)


def run_step(recompute, group):
    from pgca_amd import hip
    from pgca_amd.arch import tiny_arch
    from pgca_amd.engine import DropoutPlan
    from pgca_amd.model import PreferenceGuidedCaptioningModel
    from pgca_amd.steps import DPOStep, ReferencePolicy
    arch = tiny_arch()
    assert arch.gpt.layers == 2
    model = PreferenceGuidedCaptioningModel(freeze_vision_backbone=True, arch=arch, seed=7, device="cuda:0")
    gen = torch.Generator().manual_seed(99)
    B = len(LENS) // 2
    ids = torch.randint(0, arch.gpt.base_vocab, (2 * B, S), generator=gen)
    mask = (torch.arange(S)[None] < torch.tensor(LENS)[:, None]).long()
    batch = {"image": torch.randn(B, 3, arch.vit.image, arch.vit.image, generator=gen), "preferred_ids": ids[:B],
             "rejected_ids": ids[B:], "preferred_mask": mask[:B], "rejected_mask": mask[B:]}
    ref = ReferencePolicy(model.store, model.ws)
    for seg in ref.store.segments.values():   # a reference that differs from the policy: non-zero DPO logits
        seg.fp32.mul_(1.02)
        seg.ensure_bf16()
    step = DPOStep(model.store, model.ws, model.vision_encoder.tower, model.vision_encoder.head,
                   model.caption_decoder.engine, beta=0.1, reference_free=False, ref=ref,
                   dropout=DropoutPlan(0.1, base_seed=5), packed=True, recompute=recompute)
    p = DPOStep.prepare(batch, model.device)
    assert p["seq"].pack is not None
    for s in model.store.trainable_segments():
        s.grad.zero_()
    hip.set_option("gemm_group", group)
    try:
        loss = step.loss_and_grads(p["image"], p["seq"]).clone()
        torch.cuda.synchronize()
    finally:
        hip.set_option("gemm_group", 1)
    trunk = model.caption_decoder.engine.trunk
    saved = {(li, k): v.clone() for li in (0, arch.gpt.layers - 1) for k, v in trunk.saved[li].items()
             if isinstance(v, torch.Tensor)}
    grads = {name: seg.g(name).clone() for seg in model.store.trainable_segments() for name in seg.index}
    return dict(loss=loss, pol=model.ws.bufs["pol.seq_lp"][:2 * B].clone(), ref=model.ws.bufs["ref.seq_lp"][:2 * B].clone(),
                saved=saved, grads=grads)


@pytest.mark.parametrize("recompute", ["none", "mlp"])
def test_paired_step_equals_unpaired(recompute):
    a, b = run_step(recompute, 0), run_step(recompute, 0)      # the unpaired path twice: its own spread
    assert torch.equal(a["loss"], b["loss"]) and bool(torch.isfinite(a["loss"]).all())
    spread = {n: float((a["grads"][n] - b["grads"][n]).abs().max()) for n in a["grads"]}
    assert any(".h." in n and float(a["grads"][n].abs().max()) > 0 for n in spread)
    p = run_step(recompute, 1)
    assert torch.equal(p["loss"], a["loss"]), f"loss {float(p['loss'])} != {float(a['loss'])}"
    assert torch.equal(p["pol"], a["pol"]), "policy sequence log-probs differ"
    assert torch.equal(p["ref"], a["ref"]), "reference sequence log-probs differ"
    assert bool((p["pol"] != p["ref"]).any())
    kept = {"none": 12, "mlp": 10}[recompute]      # tensors a layer keeps (GptTrunk._KEPT)
    assert set(p["saved"]) == set(a["saved"]) and len(p["saved"]) >= 2 * kept
    # the attention kernel never touches the lse slots beyond a packed sequence's length (pgca_attention_fwd): compare
    # the written ones, [b, h, t] with t < len[b], of the real sequences
    written = (torch.arange(S)[None] < torch.tensor(LENS)[:, None])[:, None, :].to("cuda:0")
    for key in a["saved"]:
        x, y = p["saved"][key], a["saved"][key]
        if key[1] == "lse":
            n = len(LENS)
            x, y = torch.where(written, x[:n], 0), torch.where(written, y[:n], 0)
        assert torch.equal(x, y), f"saved activation {key} differs"
    for n, d0 in spread.items():
        d = float((p["grads"][n] - a["grads"][n]).abs().max())
        if ".h." in n or ".ln_f." in n:      # block parameters and ln_f: no atomics anywhere on their path
            assert d0 == 0.0, f"{n}: two unpaired runs differ by {d0}"
            assert torch.equal(p["grads"][n], a["grads"][n]), f"{n}: differs by {d}"
            continue
        # atomically accumulated (embedding tables, LM head, what the embedding backward feeds): one more draw of the
        # same reordering noise.  Its floor is the f32 format's: a reordered sum of a handful of terms moves by an ulp
        # of the running sum per swap, <= 8 ulps of the largest element here - two runs that happen to agree
        # (d0 == 0, seen on the GPU) do not show that a third will.
        floor = 8 * 2.0 ** -23 * float(a["grads"][n].abs().max())
        print(f"{n}: |paired - unpaired| {d:.3e}, unpaired vs unpaired {d0:.3e}, format floor {floor:.3e}")
        assert d <= max(2 * d0, floor), f"{n}: differs by {d}, unpaired-vs-unpaired spread {d0}, floor {floor}"
