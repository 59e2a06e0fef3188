"""The float64 references and the error bounds of ``test_step_kernels_gpu.py`` (tests/step_kernel_refs.py), proved with no
kernel involved: every reference against ``torch.autograd`` / ``torch.optim`` / ``LambdaLR`` in float64, every derived bound
against a correctly rounded float32 evaluation of the same formula (the worst ratio is asserted and printed with ``-s``),
the index references against the committed prepared batch."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import step_kernel_refs as K
from oracle import restatement as R

F64 = torch.float64
HYPER = dict(wd=0.01, b1=0.9, b2=0.999, eps=1e-8)


def rounded(**kw):
    return {k: K.r32(v) for k, v in kw.items()}


# ------------------------------------------------------------------------------------------------ AdamW
def test_adamw_reference_is_torch_adamw_and_the_restatement_in_float64():
    g = torch.Generator().manual_seed(1)
    h = rounded(lr=1e-2, **HYPER)
    p0 = (0.02 * torch.randn(300, generator=g)).double()
    w = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([w], lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"])
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    pr, mr, vr = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for t in range(1, 6):
        gr = torch.randn(300, generator=g).double() * 10.0 ** float(torch.randint(-4, 2, (1,), generator=g))
        w.grad = gr.clone()
        opt.step()
        out = K.adamw_ref(p, gr, m, v, t, h["lr"], h["wd"], h["b1"], h["b2"], h["eps"], 1.0)
        p, m, v = out["p"], out["m"], out["v"]
        R.adamw_step(pr, gr, mr, vr, t, h["lr"], h["wd"], h["b1"], h["b2"], h["eps"])
        for name, got, want in (("torch p", p, w.detach()), ("oracle p", p, pr), ("oracle m", m, mr), ("oracle v", v, vr)):
            assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max()), (name, t)


@pytest.mark.parametrize("gs", [1.0, K.r32(0.74) * 0.5])
def test_adamw_float32_evaluation_sits_inside_the_bounds(gs):
    """A correctly rounded float32 evaluation of the kernel's formula uses at most half of the case-5 bounds for every
    (t, lr) of the GPU test: the factor 4 in them is margin, not need."""
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for lr in K.ADAMW_LR:
        for t in K.ADAMW_T:
            h = rounded(lr=lr, **HYPER)
            p, g, m, v = K.adamw_state(50000, t, torch.Generator().manual_seed(t))
            ref = K.adamw_ref(p.double(), g.double(), m.double(), v.double(), t, h["lr"], h["wd"], h["b1"], h["b2"],
                              h["eps"], gs)
            got = K.adamw_f32(p, g, m, v, t, h["lr"], h["wd"], h["b1"], h["b2"], h["eps"], gs)
            for name, x in zip("pmv", got):
                err = (x.double() - ref[name]).abs()
                ratio = float(torch.where(err == 0, torch.zeros_like(err), err / ref["b" + name].clamp(min=1e-300)).max())
                worst[name] = max(worst[name], ratio)
    print(f"[adamw f32 emulation, gs {gs:.3f}] worst ratio to the bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 0.5, worst


def test_adamw_reference_fed_unrounded_betas_is_not_a_reference_of_the_kernel():
    """1 - 0.999f differs from 1 - 0.999 by 1.3e-5 relative: with the bias corrections of t = 1 (and of t = 2) the update
    of a non-zero state moves by many f32 roundings.  (From m = v = 0 at t = 1 the betas cancel: the step is lr sign(g).)"""
    assert abs((1 - K.r32(0.999)) / (1 - 0.999) - 1) > 1e-5
    p, g, m, v = (x.double() for x in K.adamw_state(1000, 2, torch.Generator().manual_seed(0)))
    h = rounded(lr=1e-2, **HYPER)
    for t in (1, 2):
        a = K.adamw_ref(p, g, m, v, t, h["lr"], h["wd"], h["b1"], h["b2"], h["eps"], 1.0)["p"]
        b = K.adamw_ref(p, g, m, v, t, h["lr"], h["wd"], 0.9, 0.999, h["eps"], 1.0)["p"]
        step = (a - p * (1 - h["lr"] * h["wd"])).abs()
        moved = float(((a - b).abs() / step).median())
        print(f"[adamw un-rounded betas, t={t}] median relative move of the step {moved:.3e} = {moved / K.EPS:.1f} x 2^-24")
        assert moved > 16 * K.EPS, moved


# ------------------------------------------------------------------------------------------------ step_control
SC = dict(max_norm=1.0, base_lr=5e-5, warmup=3, total_steps=8, sched_stride=2, beta1=0.9, beta2=0.999, grad_scale=1.0)


def test_step_control_state_machine_is_lambdalr_stepped_stride_times():
    base = K.r32(SC["base_lr"])
    w = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([w], lr=base)
    sched = torch.optim.lr_scheduler.LambdaLR(
        opt, lambda s: R.cosine_warmup_lr(1.0, s, SC["warmup"], SC["total_steps"]))
    ctrl = [0.0] * 8
    for step in range(1, 10):                       # through warm-up, the cosine, the end and four steps past it
        want_lr = opt.param_groups[0]["lr"]         # the value optimizer.step() would use
        ctrl, bound = K.step_control_ref(ctrl, [0.25], **SC)
        assert abs(ctrl[3] - want_lr) <= 1e-15 * base, (step, ctrl[3], want_lr)
        assert ctrl[6] == step and ctrl[7] == step * SC["sched_stride"] and ctrl[1] == 1.0
        assert abs(ctrl[4] - (1 - K.r32(0.9) ** step)) == 0 and abs(ctrl[5] - (1 - K.r32(0.999) ** step)) == 0
        assert ctrl[0] == 0.5 and abs(ctrl[2] - 1.0) <= 0
        assert bound[3] >= base * 8 * K.EPS and bound[6] == bound[7] == bound[1] == 0.0
        opt.step()
        for _ in range(SC["sched_stride"]):
            sched.step()
    assert ctrl[7] > SC["total_steps"] + 4 and ctrl[3] > 0.0      # HF's formula turns back up past the end


def test_step_control_state_machine_skip_rules():
    """include/pgca_hip.h: a non-finite norm or gate skips the step; slots 0-2 are still written."""
    ctrl, _ = K.step_control_ref([0.0] * 8, [4.0], **SC)
    assert ctrl[0] == 2.0 and abs(ctrl[2] - 1.0 / (2.0 + 1e-6)) < 1e-15 and ctrl[3] == 0.0 and ctrl[6] == 1.0
    for parts, gate, norm_is in (([1.0, float("nan")], None, math.isnan), ([float("inf"), 1.0], None, math.isinf),
                                 ([1.0], float("nan"), None), ([1.0], float("inf"), None)):
        new, bound = K.step_control_ref(ctrl, parts, gate=gate, **SC)
        assert new[1] == 0.0 and new[3:] == ctrl[3:] and bound[3:] == [0.0] * 5
        assert norm_is(new[0]) if norm_is else new[0] == 1.0
    new, _ = K.step_control_ref(ctrl, [1.0], gate=0.7, **SC)
    assert new[1] == 1.0 and new[6] == 2.0 and new[7] == 4.0 and new[3] == R.cosine_warmup_lr(K.r32(5e-5), 2, 3, 8)
    new, bound = K.step_control_ref(ctrl, [1e6], **dict(SC, max_norm=0.0))
    assert new[2] == 1.0 and bound[2] == 0.0
    # warmup = 0, total_steps = 1: both denominators clamp to 1
    new, _ = K.step_control_ref([0.0] * 8, [1.0], **dict(SC, warmup=0, total_steps=1, sched_stride=1))
    assert new[3] == K.r32(5e-5)
    new, _ = K.step_control_ref(new, [1.0], **dict(SC, warmup=0, total_steps=1, sched_stride=1))
    assert abs(new[3]) <= 1e-20
    # the norm: grad_scale is the float32 value, the sum is float64
    assert K.norm_from_partials([2.0 ** 40] + [1.0] * 999) == K.r32(math.sqrt(2.0 ** 40 + 999))
    assert K.norm_from_partials([9.0], 1 / 3) == K.r32(3.0 * K.r32(1 / 3))


# ------------------------------------------------------------------------------------------------ log-prob
def _logit_case(V, seed, n_rows=8):
    g = torch.Generator().manual_seed(seed)
    tgt = torch.randint(0, V, (n_rows,), generator=g)
    tgt[0], tgt[1] = 0, V - 1
    return K.logit_rows(n_rows, V, tgt, g), tgt, torch.randn(n_rows, generator=g).double()


@pytest.mark.parametrize("V", [1, 7, 65, 1000])
def test_logprob_references_are_cross_entropy_autograd(V):
    x32, tgt, g = _logit_case(V, 3)
    lp, _ = K.logprob_ref(x32.double(), tgt)
    x = x32.double().requires_grad_()
    ce = F.cross_entropy(x, tgt, reduction="none")
    assert float((lp + ce.detach()).abs().max()) <= 1e-12 * max(1.0, float(ce.detach().abs().max()))
    (-(ce * g).sum()).backward()
    dx, bound = K.logprob_bwd_ref(x32.double(), tgt, g)
    assert float((dx - x.grad).abs().max()) <= 1e-12 and bool(torch.isfinite(dx).all()) and bool((bound >= 0).all())


@pytest.mark.parametrize("V", [1, 63, 64, 65, 1000, 50257])
def test_logprob_float32_evaluation_sits_inside_the_bounds(V):
    """max-subtract, exp, sum, log in torch float32 stays inside the forward and backward bounds for every row kind, the
    rows with -inf entries included (so the bounds are not tighter than float32 allows)."""
    x32, tgt, g = _logit_case(V, 5)
    lp, b_lp = K.logprob_ref(x32.double(), tgt)
    got, lse32 = K.logprob_f32(x32, tgt)
    r_f = K.holds(f"logprob f32 V={V}", "forward", (got.double() - lp).abs(), b_lp, "4 eps23 (1 + ln V + |max| + |lse| + |x_t|)")
    dx, b_dx = K.logprob_bwd_ref(x32.double(), tgt, g)
    g32 = g.float()
    d32 = g32[:, None] * (F.one_hot(tgt, V).float() - torch.exp(x32 - lse32[:, None]))
    r_b = K.holds(f"logprob f32 V={V}", "backward", (d32.double() - dx).abs() - 2 * K.EPS * dx.abs(), b_dx,
                  "per element (g itself is rounded to f32 here: 2 eps |dx| taken off)")
    assert r_f <= 1.0 and r_b <= 1.0
    # the same with the exponential's results below the smallest normal flushed to zero, as a hardware exp2 does: inside
    # the bound only because of its underflow floor (the relative terms alone are 1e-4 of such an entry)
    p32 = torch.exp(x32 - lse32[:, None])
    tiny = p32 < K.F32_MIN_NORMAL
    d32 = g32[:, None] * (F.one_hot(tgt, V).float() - torch.where(tiny, torch.zeros_like(p32), p32))
    K.holds(f"logprob f32 V={V}", "backward, flushed exp", (d32.double() - dx).abs() - 2 * K.EPS * dx.abs(), b_dx,
            "per element + underflow floor")
    if V == 50257:
        assert bool((tiny & (p32 > 0)).any()), "the sharp rows must reach the underflow range"
        assert not bool(((d32.double() - dx).abs() <= b_dx - (1.0 + g.abs()[:, None]) * K.F32_MIN_NORMAL).all())
    kinds = [K.ROW_KINDS[i % 4] for i in range(x32.shape[0])]
    assert set(kinds) == set(K.ROW_KINDS)
    if V > 7:
        assert bool(torch.isinf(x32[3]).any()) and not bool(torch.isinf(x32[3, tgt[3]]))


# ------------------------------------------------------------------------------------------------ DPO
@pytest.mark.parametrize("dist", ["workload", "saturating", "ties"])
@pytest.mark.parametrize("ls,use_ref", [(0.0, True), (0.1, True), (0.0, False)])
def test_dpo_reference_terms_and_gradients(dist, ls, use_ref):
    B, beta, ls = 65, K.r32(0.1), K.r32(ls)
    pw, pl, rw, rl = K.dpo_inputs(B, dist, torch.Generator().manual_seed(2))
    if not use_ref:
        rw = rl = None
    ref = K.dpo_ref(pw, pl, rw, rl, beta, ls)
    assert abs(ref["term_mean"] - ref["loss"]) <= 1e-12 * max(1.0, abs(ref["loss"]))
    z = beta * ((pw.double() - pl.double()) - (0.0 if rw is None else rw.double() - rl.double()))
    dz = -((1 - ls) * (1 - torch.sigmoid(z)) - ls * torch.sigmoid(z)) / B
    assert float((ref["dpw"] - beta * dz).abs().max()) <= 1e-15 and float((ref["dpl"] + beta * dz).abs().max()) <= 1e-15
    assert bool(torch.isfinite(ref["dpw"]).all()) and ref["finite"]
    if dist == "saturating":
        assert float(z.max()) >= 59.0 and float(z.min()) <= -59.0
    if dist == "ties" and use_ref:
        assert ref["metrics"][1] == 0.0 and abs(ref["loss"] - math.log(2.0)) < 1e-12
    bad = pw.clone()
    bad[3] = float("nan")
    assert not K.dpo_ref(bad, pl, rw, rl, beta, ls)["finite"]


# ------------------------------------------------------------------------------------------------ L2 normalise
@pytest.mark.parametrize("B,P", [(1, 1), (5, 63), (4, 65), (33, 1000)])
def test_l2norm_float32_evaluation_sits_inside_the_bounds(B, P):
    g = torch.Generator().manual_seed(7)
    x = K.l2norm_rows(B, P, g)
    dy = torch.randn(B, P, generator=g)
    ref = K.l2norm_ref(x, dy)
    n32 = (x * x).sum(-1).sqrt().clamp(min=1e-12)
    y32 = x / n32[:, None]
    K.holds(f"l2norm f32 {B}x{P}", "y", (y32.double() - ref["y"]).abs(), ref["by"], "sum_bound through sqrt and quotient")
    K.holds(f"l2norm f32 {B}x{P}", "norm", (n32.double() - ref["norm"]).abs(), ref["bn"], "sum_bound through sqrt")
    yr, nr = ref["y"].float(), ref["norm"].float()
    clamped = (nr <= 1e-12)[:, None]
    t = torch.where(clamped, torch.zeros(B, 1), (dy * yr).sum(-1, keepdim=True))
    dx32 = (dy - yr * t) * (1.0 / nr)[:, None]
    K.holds(f"l2norm f32 {B}x{P}", "dx", (dx32.double() - ref["dx"]).abs(), ref["bdx"], "sum_bound of dy.y through the quotient")
    if B >= 4:      # the clamp: below 1e-12 the divisor is the constant, and autograd sends nothing through the norm
        assert float(ref["norm"][B - 1]) == K.L2_EPS and float(ref["norm"][B - 2]) == K.L2_EPS
        assert torch.equal(ref["dx"][B - 2:], dy[B - 2:].double() / K.L2_EPS) and float(ref["y"][B - 1].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ small reductions
def test_ntxent_seq_reduce_and_row_scale_references():
    g = torch.Generator().manual_seed(9)
    a, b, d = (torch.randn(257, generator=g) + s for s in (5.0, 5.0, 3.0))
    val, bound = K.ntxent_ref(a, b, d, 514)
    want = ((a.double() - d.double()).sum() + (b.double() - d.double()).sum()) / (2 * 514)
    assert abs(val - float(want)) <= 1e-12 and 0 < bound < 1e-5
    counts = torch.tensor([3, 0, 1, 65])
    tok = torch.randn(69, generator=g)
    s, bs = K.seq_reduce_ref(tok, counts, 0)
    mean, _ = K.seq_reduce_ref(tok, counts, 1)
    assert abs(float(s[3]) - float(tok[4:].double().sum())) <= 1e-12 and float(s[1]) == 0.0 and float(bs[1]) == 0.0
    assert math.isnan(float(mean[1])) and abs(float(mean[0]) - float(tok[:3].double().mean())) <= 1e-15
    seq = torch.repeat_interleave(torch.arange(4), counts)
    dseq = torch.randn(4, generator=g)
    assert torch.equal(K.row_scale_ref(dseq, seq, counts, 2), -dseq.double()[seq])
    assert torch.equal(K.row_scale_ref(dseq, seq, counts, 3), -(dseq.double() / counts.double())[seq])


def test_split_reference_reconstructs_x():
    x = K.split_inputs(5, 72, torch.Generator().manual_seed(4))
    for pattern in (0, 1):
        y = K.split_ref(x, 8, pattern)
        hi, lo = y[:5, :72].float(), (y[:5, 144:] if pattern == 0 else y[:5, 72:144]).float()
        assert torch.equal(y[:5, 72:144] if pattern == 0 else y[:5, 144:], y[:5, :72])
        assert float(((hi.double() + lo.double()) - x.double()).abs().max()) <= 2.0 ** -16 * float(x.abs().max())
        assert bool((lo[:, 0] == 0).all()) and bool((lo[:, 4] == 2.0 ** -9).all()) and not bool(y[5:].any())


# ------------------------------------------------------------------------------------------------ index builders
def test_index_references_reproduce_the_committed_prepared_batch(golden):
    g = golden("logprob_dpo")
    ids, mask = torch.from_numpy(g["ids_w"]), torch.from_numpy(g["mask_w"])
    ref = K.seq_batch_prepare_ref(ids.tolist(), mask.tolist())
    keep = mask[:, 1:] != 0
    b, t = torch.nonzero(keep, as_tuple=True)
    assert ref["targets"] == R.gather_indices(ids)[keep].tolist() and ref["counts"] == keep.sum(1).tolist()
    assert ref["row_map"] == (b * ids.shape[1] + t).tolist() and ref["seq_of_row"] == b.tolist() and ref["n"] == int(keep.sum())
    logits = torch.from_numpy(g["logits_w"])
    lp = torch.log_softmax(logits.view(-1, logits.shape[-1])[ref["row_map"]], -1).gather(
        1, torch.tensor(ref["targets"])[:, None])[:, 0]
    seq = torch.zeros(ids.shape[0]).index_add_(0, torch.tensor(ref["seq_of_row"]), lp)
    np.testing.assert_allclose(seq.numpy(), g["seq_sum_w"], atol=2e-5)


@pytest.mark.parametrize("Bq,S", [(1, 2), (5, 16), (65, 64), (7, 129)])
def test_pack_reference_is_the_documented_layout(Bq, S):
    ids, mask = K.index_batch(Bq, S, torch.Generator().manual_seed(Bq * 1000 + S))
    prep = K.seq_batch_prepare_ref(ids.tolist(), mask.tolist())
    pk = K.seq_pack_prepare_ref(prep["mask32"], S, 64, prep["counts"], prep["row_map"])
    mk = (mask != 0).numpy()
    want_len = np.array([0 if not r.any() else int(np.nonzero(r)[0].max()) + 1 for r in mk])
    cu = np.concatenate([[0], np.cumsum(want_len)])
    n = int(cu[-1])
    Mp = (n + 63) // 64 * 64
    assert pk["lens"] == want_len.tolist() and pk["n"] == n and pk["padded"] == Mp
    assert pk["F"] == (1 if S >= 63 else -(-63 // S)) and len(pk["cu"]) == Bq + pk["F"] + 1
    assert pk["cu"] == cu.tolist() + [min(n + f * S, Mp) for f in range(1, pk["F"] + 1)] and pk["cu"][-1] == Mp
    rm = np.array(prep["row_map"], dtype=np.int64)
    assert pk["row_map"] == (cu[rm // S] + rm % S).tolist() if len(rm) else pk["row_map"] == []
    assert [pk["row_ids"][r] for r in pk["row_map"]] == prep["row_map"] and pk["row_ids"][n:] == [-1] * (Mp - n)
