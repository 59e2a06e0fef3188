"""Activation recompute of the GPT-2 trunks (``GptTrunk.recompute``: ``none | mlp | block``).

Every dropout site is a counter hash of the padded position and the backward of a recompute mode replays the forward's
own launches on the saved checkpoint, so the rebuilt buffers - and with them the loss and every gradient - must equal
mode ``none`` BIT FOR BIT.  The trunk's backward has no float atomics (the grouped weight gradient takes the whole K per
tile, column sums are two-pass); the only atomically accumulated gradients of a whole step are the embedding tables and
what sits behind them, which are compared against the spread two ``none`` runs show.

Geometry: hidden 128, FOUR layers (the fewest at which a parity-alternated scratch buffer is reused - layers ``li`` and
``li + 2`` - while a side-stream weight-gradient launch is in flight), S = 128, six ragged sequences.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

LENS = [128, 40, 77, 16, 2, 100]
S = 128
MODES = ("mlp", "block")


def dev():
    return torch.device("cuda:0")


def _arch(layers=4):
    from pgca_amd.arch import VIT_ZOO, GptArch, ModelArch
    return ModelArch(vit=VIT_ZOO["tiny-vit"], gpt=GptArch(128, layers, 2, n_pos=128, base_vocab=509), proj_dim=64)


_stores = {}


def _store(layers):
    """One seeded text-tower segment per depth, shared by every run (the runs zero its gradient buffer)."""
    if layers not in _stores:
        from pgca_amd import hip
        from pgca_amd.params import ParamStore
        hip.load()
        st = ParamStore(_arch(layers), dev(), seed=3, frozen=("vit",), segments=("text_tower",))
        seg = st.segments["text_tower"]
        g = torch.Generator().manual_seed(17)   # LayerNorm gains / biases away from 1 / 0: every gradient term is live
        seg.fp32.add_(0.02 * torch.randn(seg.numel, generator=g).to(dev()))
        seg.ensure_train_state()
        seg.ensure_bf16()
        _stores[layers] = st
    return _stores[layers]


def _inputs(packed, layers=4):
    """Fixed h0 / upstream gradient and the row layout (CPU generator: the same numbers on every run)."""
    from pgca_amd.engine import make_row_pack
    Bq = len(LENS)
    mask = (torch.arange(S)[None] < torch.tensor(LENS)[:, None]).int().to(dev()).contiguous()
    pack = make_row_pack(mask) if packed else None
    M = pack.Mp if packed else Bq * S
    H = _arch(layers).gpt.hidden
    g = torch.Generator().manual_seed(29)
    h0 = torch.randn(M, H, generator=g).to(dev())
    dfeats = (0.05 * torch.randn(M, H, generator=g)).to(dev())
    if packed:                      # filler rows: zero stream, zero gradient (as the embedding kernel leaves them)
        h0[pack.n:] = 0
        dfeats[pack.n:] = 0
    return Bq, mask, pack, M, h0, dfeats


def _top(trunk, hL, rw, dfeats):
    """dL/d(stream after the last block) as the engines hand it to ``backward``: the ln_f backward's f32 ``g`` and its
    bf16 copy that carries the mask of the last layer's mlp dropout (``top_drop()``)."""
    from pgca_amd import hip
    M, H = hL.shape
    mf, rf = torch.empty(M, device=dev()), torch.empty(M, device=dev())
    feats = torch.empty(M, H, device=dev())
    hip.layernorm_fwd(hL, M, H, trunk.lnf_w.w, trunk.lnf_b.w, trunk.arch.eps, y_f32=feats, mean=mf, rstd=rf)
    g = torch.zeros(M, H, device=dev())
    g_bf = torch.zeros(M, H, dtype=torch.bfloat16, device=dev())
    part = torch.zeros(2, hip.layernorm_bwd_blocks(M), H, device=dev())
    hip.layernorm_bwd(hL, M, H, trunk.lnf_w.w, mf, rf, g, dy_f32=dfeats, dx_bf16=g_bf, part=part,
                      drop_dx=trunk.top_drop(), drop_rows=rw.ids)
    return g, g_bf


def run_trunk(mode, packed, p, overlap=True, layers=4, top=None, backwards=1):
    """Forward(save) + ``backwards`` backwards of a fresh trunk on a fresh workspace.  ``top``: the (g, g_bf) pair of
    another run (the reference's), so every mode gets the SAME upstream gradient."""
    from pgca_amd.engine import TOWER_TEXT, DropoutPlan, GptTrunk, Workspace, _rows
    st = _store(layers)
    seg = st.segments["text_tower"]
    ws = Workspace(dev())
    trunk = GptTrunk(st, "text_encoder.text_model", _arch(layers).gpt, ws, "t.trunk")
    trunk.recompute = mode
    trunk.overlap_wgrad = overlap
    assert trunk.recompute == mode
    Bq, mask, pack, M, h0, dfeats = _inputs(packed, layers)
    drop = DropoutPlan(p, base_seed=5).bind(TOWER_TEXT)
    assert (drop is None) == (p == 0.0)
    h_in = h0.clone()
    hL = trunk.forward(h_in, mask, Bq, S, True, drop, pack=pack)
    assert torch.equal(h_in, h0), "the training forward overwrote its input"
    out = dict(hL=hL.clone())
    g, g_bf = top if top is not None else _top(trunk, hL, _rows(pack, Bq, S), dfeats)
    out["top"] = (g, g_bf)
    lo, hi = trunk.layer_ranges[0][0], trunk.layer_ranges[-1][1]
    runs = []
    for _ in range(backwards):      # a later backward meets the stale contents the earlier one left in every scratch buffer
        seg.grad.zero_()
        g0 = trunk.backward(g.clone(), g_bf.clone())
        torch.cuda.synchronize()
        runs.append((g0.clone(), seg.grad[lo:hi].clone()))
    out["g0"], out["grad"] = runs[0]
    out["runs"] = runs
    out["nbytes"] = ws.nbytes()
    # every layer still exposes its input (TextEncoder.forward(return_hidden_states=True) reads it)
    assert all(trunk.saved[li]["hin"].shape == (M, h0.shape[1]) for li in range(layers))
    assert trunk.saved[0]["hin"].data_ptr() == h_in.data_ptr()
    return out


_ref = {}


def reference(packed, p):
    """Mode ``none``, computed once per (rows, dropout) and left unchanged."""
    if (packed, p) not in _ref:
        _ref[(packed, p)] = run_trunk("none", packed, p)
    return _ref[(packed, p)]


def _same(a, b, what):
    assert torch.equal(a["hL"], b["hL"]), f"{what}: hL differs"
    assert torch.equal(a["g0"], b["g0"]), f"{what}: dL/dh0 differs"
    assert torch.equal(a["grad"], b["grad"]), \
        f"{what}: {int((a['grad'] != b['grad']).sum())} of {a['grad'].numel()} trunk gradient elements differ"


# ------------------------------------------------------------------------------------------------- 1: the trunk
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "padded"])
def test_none_reproduces_itself(packed, p):
    """Guard of everything below: the trunk's backward has no float atomics, so two runs of ``none`` are bit-equal."""
    ref = reference(packed, p)
    assert bool(torch.isfinite(ref["hL"]).all()) and float(ref["grad"].abs().max()) > 0
    _same(run_trunk("none", packed, p, top=ref["top"]), ref, "none vs none")


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "padded"])
@pytest.mark.parametrize("mode", MODES)
def test_trunk_bit_for_bit(mode, packed, p):
    ref = reference(packed, p)
    _same(run_trunk(mode, packed, p, top=ref["top"]), ref, f"{mode} vs none")


# ------------------------------------------------------------------------------------------------- 2: side stream
@pytest.mark.parametrize("mode", MODES)
def test_overlap_hazard(mode):
    """The grouped weight-gradient launch of layer ``li`` reads ``ln1 / att / ln2 / act`` on the side stream while the
    main stream already rebuilds layer ``li - 1`` into scratch: overlapped == serial, and a second backward on the same
    workspace (stale scratch from the first) == the first."""
    ref = reference(True, 0.1)
    a = run_trunk(mode, True, 0.1, overlap=True, top=ref["top"], backwards=2)
    b = run_trunk(mode, True, 0.1, overlap=False, top=ref["top"])
    assert bool(torch.isfinite(a["hL"]).all())
    _same(a, b, f"{mode}: overlap_wgrad True vs False")
    _same(a, ref, f"{mode} overlapped vs none")
    (g0a, ga), (g0b, gb) = a["runs"]
    assert torch.equal(g0a, g0b) and torch.equal(ga, gb), "second backward on the same workspace differs"


# ------------------------------------------------------------------------------------------------- 3: whole steps
def _model(seed=7):
    from pgca_amd.arch import tiny_arch, with_layers
    from pgca_amd.model import PreferenceGuidedCaptioningModel
    arch = with_layers(tiny_arch(), 2, 4)
    return PreferenceGuidedCaptioningModel(freeze_vision_backbone=True, arch=arch, seed=seed, device="cuda:0"), arch


def _grads(model):
    out = {}
    for seg in model.store.trainable_segments():
        for name in seg.index:
            out[name] = seg.g(name).clone()
    return out


def _dpo(mode):
    from pgca_amd.engine import DropoutPlan
    from pgca_amd.steps import DPOStep, ReferencePolicy
    model, arch = _model()
    gen = torch.Generator().manual_seed(99)
    B, S_ = 3, 32
    lens = [32, 9, 20, 5, 17, 31]
    ids = torch.randint(0, arch.gpt.base_vocab, (2 * B, S_), generator=gen)
    mask = (torch.arange(S_)[None] < torch.tensor(lens)[:, None]).long()
    batch = {"image": torch.randn(B, 3, arch.vit.image, arch.vit.image, generator=gen), "preferred_ids": ids[:B],
             "rejected_ids": ids[B:], "preferred_mask": mask[:B], "rejected_mask": mask[B:]}
    ref = ReferencePolicy(model.store, model.ws)
    for seg in ref.store.segments.values():   # a reference that differs from the policy: non-zero DPO logits
        seg.fp32.mul_(1.02)
        seg.ensure_bf16()
    kw = {} if mode is None else {"recompute": mode}
    step = DPOStep(model.store, model.ws, model.vision_encoder.tower, model.vision_encoder.head,
                   model.caption_decoder.engine, beta=0.1, reference_free=False, ref=ref,
                   dropout=DropoutPlan(0.1, base_seed=5), packed=True, **kw)
    assert model.caption_decoder.engine.trunk.recompute == (mode or "none")
    p = DPOStep.prepare(batch, model.device)
    for s in model.store.trainable_segments():
        s.grad.zero_()
    loss = step.loss_and_grads(p["image"], p["seq"]).clone()
    torch.cuda.synchronize()
    return loss, _grads(model)


def _contrastive(mode):
    from pgca_amd.engine import DropoutPlan
    from pgca_amd.steps import ContrastiveStep
    model, arch = _model()
    assert model.store.segments["text_tower"].trainable
    gen = torch.Generator().manual_seed(78)
    B, S_ = 4, 32
    ids = torch.randint(0, arch.gpt.base_vocab, (B, S_), generator=gen)
    mask = (torch.arange(S_)[None] < torch.tensor([32, 9, 20, 5])[:, None]).long()
    batch = {"image": torch.randn(B, 3, arch.vit.image, arch.vit.image, generator=gen), "caption_ids": ids,
             "caption_mask": mask}
    kw = {} if mode is None else {"recompute": mode}
    step = ContrastiveStep(model.store, model.ws, model.vision_encoder.tower, model.vision_encoder.head,
                           model.text_encoder.engine, temperature=0.5, dropout=DropoutPlan(0.1, base_seed=5), **kw)
    assert model.text_encoder.engine.trunk.recompute == (mode or "none")
    p = ContrastiveStep.prepare(batch, model.device)
    for s in model.store.trainable_segments():
        s.grad.zero_()
    loss = step.loss_and_grads(p["image"], p["ids"], p["mask"], pack=p["pack"]).clone()
    torch.cuda.synchronize()
    return loss, _grads(model)


def _atomic_class_allowed(name):
    """Gradients that may differ between two identical runs: the atomically accumulated embedding tables and what the
    embedding backward feeds (the decoder's prefix path, the projection heads).  Never a block parameter or ln_f."""
    return ".h." not in name and ".ln_f." not in name


@pytest.mark.parametrize("step", [_dpo, _contrastive], ids=["dpo4", "contrastive"])
def test_whole_step(step):
    loss_a, ga = step(None)          # the default argument: mode none
    loss_b, gb = step("none")
    assert torch.equal(loss_a, loss_b) and bool(torch.isfinite(loss_a).all())
    spread = {}
    for name in ga:
        d = float((ga[name] - gb[name]).abs().max())
        assert d == 0.0 or _atomic_class_allowed(name), f"{name}: two runs of mode none differ by {d}"
        spread[name] = d
    assert any(".h." in n and float(ga[n].abs().max()) > 0 for n in ga)
    for mode in MODES:
        loss_m, gm = step(mode)
        assert torch.equal(loss_m, loss_a), f"{mode}: loss {float(loss_m)} != {float(loss_a)}"
        for name in ga:
            d = float((gm[name] - ga[name]).abs().max())
            if spread[name] == 0.0:
                assert torch.equal(gm[name], ga[name]), f"{mode}: {name} differs by {d}"
            else:
                print(f"{mode} {name}: |diff| {d:.3e}, none-vs-none {spread[name]:.3e}")
                assert d <= 4 * spread[name], f"{mode}: {name} differs by {d}, none-vs-none spread {spread[name]}"


# ------------------------------------------------------------------------------------------------- 4: memory
def test_workspace_growth_per_layer():
    """Bytes one more layer costs, from the table of what each mode keeps per row (H = hidden): ``block`` one f32
    checkpoint row (4H), ``mlp`` hin + ln1 + qkv + att + hm = 18H, ``none`` 36H; + the row statistics and lse."""
    M, H = len(LENS) * S, 128
    assert M == 768
    grow = {mode: run_trunk(mode, False, 0.0, layers=8)["nbytes"] - run_trunk(mode, False, 0.0, layers=4)["nbytes"]
            for mode in ("none", "mlp", "block")}
    print("workspace bytes of 4 more layers:", grow, "per row and layer:", {k: v / (4 * M) for k, v in grow.items()})
    assert grow["block"] <= 4 * M * (4 * H + 64)
    assert grow["mlp"] <= 4 * M * (18 * H + 64)
    assert grow["none"] > 4 * M * 32 * H


# ------------------------------------------------------------------------------------------------- 5: arguments
def test_unknown_mode_raises():
    from pgca_amd.engine import GptTrunk, Workspace
    from pgca_amd.steps import ContrastiveStep, DPOStep
    trunk = GptTrunk(_store(4), "text_encoder.text_model", _arch(4).gpt, Workspace(dev()), "t.trunk")
    assert trunk.recompute == "none"
    with pytest.raises(ValueError):
        trunk.recompute = "bogus"
    assert trunk.recompute == "none"
    model, _ = _model()
    with pytest.raises(ValueError):
        DPOStep(model.store, model.ws, model.vision_encoder.tower, model.vision_encoder.head,
                model.caption_decoder.engine, reference_free=True, recompute="bogus")
    with pytest.raises(ValueError):
        ContrastiveStep(model.store, model.ws, model.vision_encoder.tower, model.vision_encoder.head,
                        model.text_encoder.engine, temperature=0.5, recompute="bogus")
