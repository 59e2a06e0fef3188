"""Plain float64 references, error bounds and input makers of the small kernels of a training step (csrc/misc.hip): the
DPO loss, the materialised-logits log-prob, L2 normalise, the NT-Xent scalar, the hi/lo bf16 split, the sequence reduce,
the batch index builders, the optimiser chain and the ViT input kernels.  Shared by ``test_step_kernels_gpu.py`` (which
runs them next to the kernels) and ``test_step_kernel_references_cpu.py`` (which proves the references against
``torch.autograd`` / ``torch.optim`` and the bounds against a correctly rounded float32 evaluation, with no kernel
involved).

Nothing here knows about blocks, waves or grid strides, with one exception: ``SQ_BLOCK`` / ``SWEEP``, the documented
work of one ``sqnorm`` block and of one grid sweep, which decide WHERE a test looks, never what it expects.

The C ABI takes every hyper-parameter as ``float``.  ``1 - 0.999f ** t`` differs from ``1 - 0.999 ** t`` by 1.3e-5
relative at t = 1, orders above the f32 rounding of an update, so every reference here is fed ``r32(x)``, the float32
value the kernel receives, never the Python double.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import restatement as R
from row_kernel_refs import bf16_round, sum_bound

F64 = torch.float64
EPS = 2.0 ** -24            # unit roundoff of float32 (half an ulp of 1)
EPS23 = 2.0 ** -23
F32_MIN_NORMAL = 2.0 ** -126
SQ_BLOCK = 16384            # elements of one pgca_sqnorm partial (include/pgca_hip.h: pgca_sqnorm_blocks)
SWEEP = 8192 * 256          # threads of one capped grid sweep of the flat optimiser kernels (x 4 or x 8 elements each)


def r32(x):
    """The float32 value a ``float`` argument of the C ABI carries, as a Python double."""
    return float(np.float32(x))


def ulp32(x):
    """Spacing of float32 at |x| (float64 tensor of the same shape); the smallest normal's below 2^-126."""
    x = torch.as_tensor(x, dtype=F64).abs().clamp(min=2.0 ** -126)
    _, e = torch.frexp(x)
    return torch.ldexp(torch.ones_like(x), e - 24)


def report(case, what, measured, bound, source):
    print(f"[{case}] {what}: measured {measured:.3e}  bound {bound:.3e}  ({source})")


def holds(case, what, err, bound, source):
    """err, bound: tensors of one shape or floats; asserts err <= bound everywhere (a NaN error fails) and prints the entry
    closest to its bound.  Returns the worst ratio.  As ``holds`` of test_bench_geometry_rows_gpu.py, but an entry may be
    EXACT here (bound 0 and error 0: ratio 0), and this module must import without a GPU test module."""
    err = torch.as_tensor(err, dtype=F64)
    bound = torch.as_tensor(bound, dtype=F64, device=err.device).expand_as(err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300)).flatten()
    worst = int(torch.nan_to_num(ratio, nan=float("inf")).argmax()) if ratio.numel() else 0
    w = float(ratio[worst]) if ratio.numel() else 0.0
    report(case, what, float(err.flatten()[worst]) if ratio.numel() else 0.0,
           float(bound.flatten()[worst]) if ratio.numel() else 0.0, f"{source}; worst entry {worst} at {w:.3f} of its bound")
    assert bool((err <= bound).all()), f"[{case}] {what}: entry {worst} is at {w:.3f} x its bound ({source})"
    return w


def scalar_matches(got, ref, bound):
    """A float32 scalar against its reference: NaN for NaN, the same infinity for an infinity, else |got - ref| <= bound."""
    if math.isnan(ref):
        return math.isnan(got)
    if math.isinf(ref):
        return got == ref
    return abs(got - ref) <= bound


# ------------------------------------------------------------------------------------------------ sqnorm / norm
def sqnorm_ref(g):
    """float64 sum of squares of every ``SQ_BLOCK`` slice of the flat f32 buffer g, and the slices' lengths."""
    n = g.numel()
    nb = (n + SQ_BLOCK - 1) // SQ_BLOCK
    sq = torch.zeros(nb * SQ_BLOCK, dtype=F64, device=g.device)
    sq[:n] = g.double() ** 2
    lens = torch.full((nb,), float(SQ_BLOCK), dtype=F64, device=g.device)
    lens[-1] = n - (nb - 1) * SQ_BLOCK
    return sq.view(nb, SQ_BLOCK).sum(1), lens


def sqnorm_bound(part, lens):
    """sum_bound(min(16384, len), sum g^2): the terms are squares, so sum |terms| is the partial itself."""
    return sum_bound(lens.clamp(max=SQ_BLOCK), part)


def norm_from_partials(parts, grad_scale=1.0):
    """float32(sqrt(sum_f64(parts) * float64(float32(grad_scale))^2)) as a Python float; NaN / inf pass through."""
    s = math.fsum(float(x) for x in parts)
    if math.isnan(s) or math.isinf(s):
        return s
    return r32(math.sqrt(s * r32(grad_scale) ** 2))


# ------------------------------------------------------------------------------------------------ step_control
def step_control_ref(ctrl, parts, max_norm, base_lr, warmup, total_steps, sched_stride, beta1, beta2, grad_scale,
                     gate=None):
    """One ``pgca_step_control`` call as a Python / float64 state machine (include/pgca_hip.h): ``ctrl`` is the list of the
    eight slots before the call.  Returns (slots after, absolute bound of every slot; 0 = exact).

    * [0] norm, [1] finite flag, [2] clip are written by every call; the step is SKIPPED when the norm or ``gate`` is not
      finite, and then slots 3-7 keep their values;
    * a taken step reads lr from the schedule BEFORE the counters advance (optimizer.step() then scheduler.step()); the
      schedule is ``oracle.restatement.cosine_warmup_lr`` (HF's formula, unclamped past total_steps), advanced
      ``sched_stride`` per optimiser step;
    * bias corrections 1 - beta^t from the float32-rounded betas.
    Bounds: norm and clip 2 f32 ulp; lr base_lr * 8 * 2^-24 * (1 + pi * prog) (f32 prog, the f32 pi product, cosf);
    bias corrections 4 * 2^-24 * beta^t (4 ulp of powf's result; the subtraction from 1 is exact above 0.5); counters exact.
    """
    norm = norm_from_partials(parts, grad_scale)
    finite = math.isfinite(norm) and (gate is None or math.isfinite(gate))
    new, bound = list(ctrl), [0.0] * 8
    new[0] = norm
    bound[0] = 2 * float(ulp32(norm)) if math.isfinite(norm) else 0.0
    new[1] = 1.0 if finite else 0.0
    if not max_norm > 0 or math.isnan(norm):
        new[2] = 1.0                                 # max_norm = 0: no clipping; fminf(1, NaN) = 1
    elif math.isinf(norm):
        new[2] = 0.0
    else:
        new[2] = R.clip_coefficient(norm, r32(max_norm))
        bound[2] = 2 * float(ulp32(new[2]))
    if finite:
        sched, step = int(ctrl[7]), int(ctrl[6]) + 1
        new[3] = R.cosine_warmup_lr(r32(base_lr), sched, warmup, total_steps)
        prog = max(0.0, (sched - warmup) / max(1, total_steps - warmup))
        bound[3] = r32(base_lr) * 8 * EPS * (1 + math.pi * prog)
        new[4], new[5] = 1.0 - r32(beta1) ** step, 1.0 - r32(beta2) ** step
        bound[4], bound[5] = 4 * EPS * r32(beta1) ** step, 4 * EPS * r32(beta2) ** step
        new[6], new[7] = float(step), float(sched + sched_stride)
    return new, bound


# ------------------------------------------------------------------------------------------------ AdamW
ADAMW_T = (1, 2, 10, 1000, 100000)
ADAMW_LR = (5e-5, 1e-2)


def adamw_state(n, t, gen):
    """One random f32 optimiser state: p ~ 0.02 N(0,1); m, g signed with log-uniform magnitude over e^-12 .. e^2; v >= 0
    over e^-24 .. e^4 (scaled down for young states, as a real second moment is); m = v = 0 at t = 1."""
    d = gen.device
    rn = lambda: torch.randn(n, generator=gen, device=d, dtype=F64)                    # noqa: E731
    lu = lambda lo, hi: torch.exp(torch.rand(n, generator=gen, device=d, dtype=F64) * (hi - lo) + lo)   # noqa: E731
    p = (0.02 * rn()).float()
    g = (rn() * lu(-12, 2)).float()
    if t == 1:
        return p, g, torch.zeros_like(p), torch.zeros_like(p)
    m = (0.3 * rn() * lu(-12, 2)).float()
    v = (rn().abs() * lu(-24, 4) * min(1.0, t * 0.001)).float()
    return p, g, m, v


def adamw_ref(p, g, m, v, t, lr, wd, b1, b2, eps, gs):
    """The kernel's formula in float64; p, g, m, v float64 tensors, every scalar ALREADY the float32 value the kernel is
    given (``r32``), gs = clip * grad_scale.  Returns dict(p, m, v, bp, bm, bv): results and absolute bounds.

    With e = 2^-24 and abs_m = b1 |m| + (1 - b1) |g gs|:  m: 4 * 3e abs_m;  v: 4 * 4e v;
    p: 4 * [2e |p| + (2e/bc2 + 2e/bc1 + 12e) (lr/bc1) abs_m / denom]  - the bias corrections come from powf (their absolute
    error e-ish is relative e/bc), the rest are the roundings of the chain; abs_m instead of |m'| because m and g cancel.
    The factor 4 is margin over a correctly rounded f32 evaluation (test_step_kernel_references_cpu.py)."""
    gg = g * gs
    w = p * (1.0 - lr * wd)
    m2 = b1 * m + (1.0 - b1) * gg
    v2 = b2 * v + (1.0 - b2) * gg * gg
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    denom = v2.sqrt() / math.sqrt(bc2) + eps
    p2 = w - (lr / bc1) * (m2 / denom)
    abs_m = b1 * m.abs() + (1.0 - b1) * gg.abs()
    return dict(p=p2, m=m2, v=v2, bm=4 * 3 * EPS * abs_m, bv=4 * 4 * EPS * v2,
                bp=4 * (2 * EPS * p2.abs() + (2 * EPS / bc2 + 2 * EPS / bc1 + 12 * EPS) * (lr / bc1) * abs_m / denom))


def adamw_f32(p, g, m, v, t, lr, wd, b1, b2, eps, gs):
    """The same formula with every operation rounded to float32 (torch CPU float32, powf for the bias corrections): what a
    correct kernel computes up to fused multiply-adds."""
    f = lambda x: torch.tensor(x, dtype=torch.float32)                                 # noqa: E731
    lr, wd, b1, b2, eps, gs, one = f(lr), f(wd), f(b1), f(b2), f(eps), f(gs), f(1.0)
    bc1, bc2 = one - torch.pow(b1, f(float(t))), one - torch.pow(b2, f(float(t)))
    gg = g * gs
    w = p * (one - lr * wd)
    m2 = b1 * m + (one - b1) * gg
    v2 = b2 * v + (one - b2) * gg * gg
    denom = v2.sqrt() / bc2.sqrt() + eps
    return w - (lr / bc1) * (m2 / denom), m2, v2


# ------------------------------------------------------------------------------------------------ DPO loss
def dpo_inputs(B, dist, gen):
    """pol_w, pol_l, ref_w, ref_l f32 [B]: ``workload`` log-probs in -200 .. -5 whose differences are a few units;
    ``saturating``: pol - ref spans +-600, so z = 0.1 (pol - ref) spans +-60; ``ties``: pol == ref exactly."""
    d = gen.device
    u = lambda: torch.rand(B, generator=gen, device=d)                                 # noqa: E731
    n = lambda: torch.randn(B, generator=gen, device=d)                                # noqa: E731
    base = -200.0 + 195.0 * u()
    if dist == "workload":
        return base + 2 * n(), base + 2 * n(), base + 2 * n(), base + 2 * n()
    if dist == "saturating":
        gap = torch.linspace(-600.0, 600.0, B, device=d) if B > 1 else torch.full((1,), 600.0, device=d)
        gap = gap[torch.randperm(B, generator=gen, device=d)]
        rw = -100.0 + n()
        return -320.0 + gap / 2, -320.0 - gap / 2, rw, rw.clone()
    pw, pl = base + 2 * n(), base + 2 * n()
    return pw, pl, pw.clone(), pl.clone()


def dpo_ref(pw, pl, rw, rl, beta, ls):
    """``oracle.restatement.dpo_loss`` in float64 with autograd (beta, ls: the float32 values).  Returns dict(loss, dpw,
    dpl, metrics [4], b_loss, b_metrics [4], finite).  Bounds: sum_bound(B, sum |term|) / B plus the per-term figure of
    test_seq_reduce_dpo_and_row_scale, 1e-5 * max(1, |value|)."""
    B = pw.numel()
    a, b = pw.double().clone().requires_grad_(), pl.double().clone().requires_grad_()
    c, d = (None, None) if rw is None else (rw.double(), rl.double())
    loss, met = R.dpo_loss(a, b, c, d, beta=beta, reference_free=rw is None, label_smoothing=ls)
    out = dict(loss=float(loss.detach()), finite=math.isfinite(float(loss.detach())))
    if out["finite"]:
        loss.backward()
        out["dpw"], out["dpl"] = a.grad, b.grad
    with torch.no_grad():
        marg = (a - b) - (0.0 if c is None else c - d)
        z = beta * marg
        term = -((1.0 - ls) * F.logsigmoid(z) + ls * F.logsigmoid(-z))
        out["term_mean"] = float(term.mean())
        terms = (term, marg, (marg > 0).double(), a.detach(), b.detach())
        vals = [out["loss"], met["reward_margin"], met["reward_accuracy"], met["policy_chosen_logprob"],
                met["policy_rejected_logprob"]]
        bnd = [float(sum_bound(B, t.abs().sum())) / B + 1e-5 * max(1.0, abs(v)) if math.isfinite(v) else 0.0
               for t, v in zip(terms, vals)]
    out["metrics"], out["b_loss"], out["b_metrics"] = vals[1:], bnd[0], bnd[1:]
    return out


# ------------------------------------------------------------------------------------------------ logits log-prob
ROW_KINDS = ("normal", "sharp", "offset", "neginf")


def logit_rows(n_rows, V, targets_of_row, gen):
    """[n_rows, V] f32 logits, row i of kind ROW_KINDS[i % 4]: normal 2 N(0,1); sharp: one logit 80 above the rest (the
    target's column on every other sharp row); offset: all logits + 1e4; neginf: a third of the entries -inf, never the
    column ``targets_of_row[i]`` (the token the row scores), never all of them."""
    d = gen.device
    x = 2.0 * torch.randn(n_rows, V, generator=gen, device=d)
    for i in range(n_rows):
        kind, t = ROW_KINDS[i % 4], int(targets_of_row[i])
        if kind == "sharp":
            x[i, t if (i // 4) % 2 == 0 else (t + V // 2) % V] += 80.0
        elif kind == "offset":
            x[i] += 1e4
        elif kind == "neginf":
            hole = torch.rand(V, generator=gen, device=d) < 1.0 / 3
            hole[t] = False
            x[i, hole] = float("-inf")
    return x


def logprob_ref(rows, targets):
    """rows float64 [R, V] (the scored rows, gathered), targets int64 [R]: shift -> log_softmax -> gather of the restatement,
    fed one sequence whose position r + 1 holds token targets[r].  Returns lp [R] and the forward bound

        4 * 2^-23 * (1 + ln V + |max| + |lse| + |logit_tgt|)

    (``__expf`` is exp2 of an f32 product: relative error 2^-23 + |x| 2^-24, weighted over the softmax sum p |x| <= ln V;
    ``__logf`` adds 2^-23 |log s| <= 2^-23 ln V; the final additions one ulp each of |max|, |lse|, |logit_tgt|)."""
    nR, V = rows.shape
    logits = torch.cat([rows, rows.new_zeros(1, V)])[None]
    labels = torch.cat([targets.new_zeros(1), targets])[None]
    lp = R.token_logprobs(logits, labels)[0]
    mx = rows.amax(-1)
    lse = torch.logsumexp(rows, -1)
    xt = rows.gather(1, targets[:, None])[:, 0]
    return lp, 4 * logprob_unit(V, mx, lse, xt)


def logprob_unit(V, mx, lse, xt):
    return EPS23 * (1.0 + math.log(V) + mx.abs() + lse.abs() + xt.abs())


def logprob_bwd_ref(rows, targets, g):
    """d (sum_r g[r] lp[r]) / d rows by autograd, [R, V] float64, and the per-element bound
    4 |g| (p_c (unit forward bound + 2^-23 (2 + |x_c - lse|)) + 2^-24 |onehot - p_c|) + (1 + |g|) 2^-126.
    The last term is the float32 underflow floor: every term before it is RELATIVE to p_c, but a p_c below the smallest
    normal 2^-126 (a logit 87.3 below the lse, which a sharp row has) is flushed to zero by the hardware exponential, and
    so may be its product with g (test_step_kernel_references_cpu.py evaluates exactly that in float32)."""
    x = rows.clone().requires_grad_()
    lp = torch.log_softmax(x, -1).gather(1, targets[:, None])[:, 0]
    (lp * g).sum().backward()
    with torch.no_grad():
        lse = torch.logsumexp(rows, -1)
        p = torch.exp(rows - lse[:, None])
        onehot = F.one_hot(targets, rows.shape[1]).to(F64)
        unit = logprob_unit(rows.shape[1], rows.amax(-1), lse, rows.gather(1, targets[:, None])[:, 0])[:, None]
        dist = torch.where(p > 0, (rows - lse[:, None]).abs(), torch.zeros_like(p))      # -inf entries: p = 0 exactly
        bound = 4 * g.abs()[:, None] * (p * (unit + EPS23 * (2.0 + dist)) + EPS * (onehot - p).abs())
        bound = bound + (1.0 + g.abs()[:, None]) * F32_MIN_NORMAL
    return x.grad, bound


def logprob_f32(rows32, targets):
    """max-subtract, exp, sum, log in torch float32: the evaluation the bounds must contain."""
    mx = rows32.amax(-1, keepdim=True)
    s = torch.exp(rows32 - mx).sum(-1)
    lse = mx[:, 0] + torch.log(s)
    return rows32.gather(1, targets[:, None])[:, 0] - lse, lse


# ------------------------------------------------------------------------------------------------ L2 normalise
L2_EPS = r32(1e-12)          # the kernel clamps the norm with the FLOAT 1e-12f


def l2norm_rows(B, P, gen):
    """[B, P] f32 unit normals; row B-1 (B >= 4) is all zero and row B-2 has norm 1e-14, below the clamp."""
    x = torch.randn(B, P, generator=gen, device=gen.device)
    if B >= 4:
        x[B - 1] = 0.0
        x[B - 2] *= 1e-14 / float(x[B - 2].double().norm())
    return x


def l2norm_ref(x, dy):
    """float64 ``F.normalize`` (eps = the float 1e-12f) with autograd.  Returns dict(y, norm, dx, by, bn, bdx).

    Forward: s = sum x^2 carries d = sum_bound(P, s) / s; n = sqrt(s) half of that plus its rounding; y = x / n one more
    rounding; one more for the products: |dy| <= |y| (d/2 + 3e), |dn| <= n (d/2 + 2e)  (e = 2^-24; a clamped norm is exact).
    Backward dx = (dy - y t) / n with t = sum dy y, fed the f32-ROUNDED reference y and n (e/2 each):
    |dt| <= sum_bound(P, sum |dy y|) + e sum |dy y|, the numerator adds e (|dy| + 3 |y t|), the quotient 3e |dx|."""
    P = x.shape[1]
    a = x.double().clone().requires_grad_()
    y = F.normalize(a, p=2, dim=-1, eps=L2_EPS)
    y.backward(dy.double())
    with torch.no_grad():
        s = (a * a).sum(-1)
        n = s.sqrt().clamp(min=L2_EPS)
        d = torch.where(s > 0, sum_bound(P, s) / s.clamp(min=1e-300), torch.zeros_like(s))
        by = y.abs() * (d[:, None] / 2 + 3 * EPS)
        bn = torch.where(n > L2_EPS, n * (d / 2 + 2 * EPS), torch.zeros_like(n))
        dyy = dy.double() * y
        t = dyy.sum(-1, keepdim=True)
        dt = (sum_bound(P, dyy.abs().sum(-1)) + EPS * dyy.abs().sum(-1))[:, None]
        bdx = (y.abs() * dt + EPS * (dy.double().abs() + 3 * (y * t).abs())) / n[:, None] + 3 * EPS * a.grad.abs()
    return dict(y=y.detach(), norm=n, dx=a.grad, by=by, bn=bn, bdx=bdx)


# ------------------------------------------------------------------------------------------------ NT-Xent scalar
def ntxent_ref(lse_r, lse_c, diag, n_total):
    """(sum (lse_r - diag) + sum (lse_c - diag)) / (2 n_total) in float64; bound: sum_bound of the 2 n_local terms / that."""
    a, b = lse_r.double() - diag.double(), lse_c.double() - diag.double()
    n = a.numel()
    return float((a + b).sum()) / (2.0 * n_total), float(sum_bound(2 * n, a.abs().sum() + b.abs().sum())) / (2.0 * n_total)


# ------------------------------------------------------------------------------------------------ sequence reduce
def seq_reduce_ref(tok, counts, mode):
    """tok f32 [nrows] sorted by sequence, counts int [nseq]: float64 sum (mode 0) or mean (mode 1; 0/0 = NaN) of every
    sequence and its bound sum_bound(count, sum |tok|) (+ one rounding of the quotient in mode 1)."""
    nseq = counts.numel()
    seq = torch.repeat_interleave(torch.arange(nseq, device=tok.device), counts.long())
    s = torch.zeros(nseq, dtype=F64, device=tok.device).index_add_(0, seq, tok.double())
    sa = torch.zeros(nseq, dtype=F64, device=tok.device).index_add_(0, seq, tok.double().abs())
    bound = sum_bound(counts.to(F64), sa)
    if mode:
        c = counts.to(F64)
        return s / c, bound / c.clamp(min=1.0) + EPS * (s / c.clamp(min=1.0)).abs()
    return s, bound


def row_scale_ref(dseq, seq_of_row, counts, mode):
    """float64 dseq[q] (mode bit 0: / count[q]; bit 1: negated) of every row."""
    q = seq_of_row.long()
    v = dseq.double()[q]
    if mode & 1:
        v = v / counts.double()[q]
    return -v if mode & 2 else v


# ------------------------------------------------------------------------------------------------ batch index builders
def seq_batch_prepare_ref(ids, mask):
    """Plain loops over ids / mask (lists of Bq lists of S ints): the shift, mask product and gather index of the
    reference's loss (labels[:, 1:] at mask[:, 1:] != 0).  Returns dict(counts, mask32, row_map, targets, seq_of_row, n)."""
    S = len(ids[0])
    counts, mask32, row_map, targets, seq_of_row = [], [], [], [], []
    for b, (row, mrow) in enumerate(zip(ids, mask)):
        c = 0
        mask32.append([1 if x != 0 else 0 for x in mrow])
        for t in range(S - 1):
            if mrow[t + 1] != 0:
                row_map.append(b * S + t)
                targets.append(row[t + 1])
                seq_of_row.append(b)
                c += 1
        counts.append(c)
    return dict(counts=counts, mask32=mask32, row_map=row_map, targets=targets, seq_of_row=seq_of_row, n=len(row_map))


def seq_pack_prepare_ref(mask32, S, pad_to, counts=None, row_map=None):
    """Plain loops: the packed row layout documented at pgca_seq_pack_prepare.  Returns dict(lens, cu [Bq+F+1], row_ids
    [padded], n, padded, F, row_map (packed numbers of the compact rows, or None))."""
    Bq = len(mask32)
    lens = [max([t + 1 for t in range(S) if row[t] != 0], default=0) for row in mask32]
    cu = [0]
    row_ids = []
    for b in range(Bq):
        cu.append(cu[-1] + lens[b])
        row_ids += [b * S + t for t in range(lens[b])]
    n = cu[-1]
    padded = (n + pad_to - 1) // pad_to * pad_to
    F_ = (pad_to - 1 + S - 1) // S
    cu += [min(n + f * S, padded) for f in range(1, F_ + 1)]
    row_ids += [-1] * (padded - n)
    packed = None
    if row_map is not None:
        packed, r = [], 0
        for b in range(Bq):
            for _ in range(counts[b]):
                packed.append(row_map[r] + cu[b] - b * S)
                r += 1
    return dict(lens=lens, cu=cu, row_ids=row_ids, n=n, padded=padded, F=F_, row_map=packed)


def index_batch(Bq, S, gen, full=False):
    """ids (up to 2^40) and an int64 mask with holes, empty sequences, mask[b, 0] = 0 and the non-zero entries 2 and -1
    (kept like a 1), as CPU int64 tensors.  ``full``: every position kept."""
    ids = torch.randint(0, 1 << 40, (Bq, S), generator=gen, dtype=torch.int64)
    ids[0, S - 1] = (1 << 40) - 1
    if full:
        return ids, torch.ones(Bq, S, dtype=torch.int64)
    lens = torch.randint(0, S + 1, (Bq,), generator=gen)
    mask = (torch.arange(S)[None] < lens[:, None]).long()
    mask[torch.rand(Bq, S, generator=gen) < 0.1] = 0                  # holes
    mask[0] = 1
    mask[0, 0] = 0
    mask[0, S - 1] = 2
    if S > 2:
        mask[0, 1] = -1
    if Bq > 2:
        mask[1] = 0                                                   # empty
        mask[2] = 0
        mask[2, 0] = 1                                                # one real token: no scored row
        mask[Bq - 1] = 1
    return ids, mask


# ------------------------------------------------------------------------------------------------ casts / split / ViT
def split_ref(x, rows_out, pattern):
    """hi = bf16(x), lo = bf16(x - hi) of x f32 [R, P] as bf16 [rows_out, 3P]: [hi | hi | lo] (pattern 0) or [hi | lo | hi]
    (pattern 1); rows R.. are zero.  x - hi is exact in float32 (hi keeps the leading 8 bits of x)."""
    R_, P = x.shape
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    y = torch.zeros(rows_out, 3 * P, dtype=torch.bfloat16, device=x.device)
    y[:R_] = torch.cat([hi, hi, lo] if pattern == 0 else [hi, lo, hi], 1)
    return y


def split_inputs(R_, P, gen):
    """Unit normals with, in every row, values whose lo is exactly 0 (bf16-representable), f32 denormals and a zero."""
    x = torch.randn(R_, P, generator=gen, device=gen.device)
    x[:, 0] = x[:, 0].bfloat16().float()
    x[:, 1] = 1e-41
    x[:, 2] = -3e-39
    x[:, 3] = 0.0
    x[:, 4] = 1.0 + 2.0 ** -9
    return x


def patchify_ref(px, P, ld):
    """bf16 of torch's unfold: [B G G, ld] with columns (c, ky, kx) and zero columns 3 P P .. ld-1."""
    B = px.shape[0]
    cols = F.unfold(px, kernel_size=P, stride=P).transpose(1, 2).reshape(-1, 3 * P * P)
    out = torch.zeros(cols.shape[0], ld, dtype=torch.bfloat16, device=px.device)
    out[:, :3 * P * P] = cols.bfloat16()
    assert cols.shape[0] == B * (px.shape[-1] // P) ** 2
    return out


def vit_assemble_ref(pe, cls, pos, B, T, H):
    return torch.cat([cls.expand(B, 1, H), pe.view(B, T - 1, H)], 1) + pos[None]


def vit_assemble_bwd_ref(dx, dcls0, dpos0):
    """dx f32 [B, T, H]; float64 dpos = dpos0 + sum_b dx, dcls = dcls0 + sum_b dx[:, 0], their bound sum_bound(B, sum_b |dx|)
    and the exact bf16 patch rows (as float64)."""
    d = dx.double()
    s, sa = d.sum(0), d.abs().sum(0)
    bound = sum_bound(dx.shape[0], sa)
    return dict(dpatch=bf16_round(d[:, 1:]).reshape(-1, dx.shape[2]), dpos=dpos0.double() + s,
                dcls=dcls0.double() + s[0], b_dpos=bound, b_dcls=bound[0])
