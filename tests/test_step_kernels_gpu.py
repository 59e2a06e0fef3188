"""The small kernels of a training step (csrc/misc.hip) on every code path, against the plain float64 references of
tests/step_kernel_refs.py (themselves proved on the CPU by test_step_kernel_references_cpu.py), inside sentinel-filled
buffers (``Guard``; ``IntGuard`` for the integer outputs).  Every shape is the smallest that reaches the branch it names.

Which case launches which kernel / branch:

===========================================  ==============================================================================
case                                         kernels and branches
===========================================  ==============================================================================
test_sqnorm_partials[n]                      sqnorm_kernel: scalar tail only (1, 3), one float4 (4), float4 + tail (5), last
                                             float4 of a block missing / present (16383, 16384), a second block of one element
                                             (16385), four blocks with a five-element last one (3 * 16384 + 5)
test_norm_from_partials[nparts]              partials_norm in step_control_kernel (ctrl[0]) and clip_coef_kernel (coef[1]):
                                             one trip, 255 / 256 / 257 (second trip of one thread), 1000; f64 sum; NaN, inf
test_step_control_state_machine              step_control_kernel: warm-up, cosine, end of schedule, past it (prog > 1), NaN /
                                             inf norm, gate NaN / inf / finite, max_norm = 0; warmup = 0 and total_steps = 1
test_clip_coef_and_scale_dev[n]              clip_coef_kernel (below / above max_norm, NaN, inf), scale_dev_kernel: early
                                             return, one float4, part block, second grid sweep (8388608 + 1088)
test_adamw_single_step[t-lr]                 adamw_kernel from a random state, bias corrections of t = 1 .. 100000; skipped
                                             step (ctrl[1] = 0); no bf16 mirror
test_adamw_second_sweep                      adamw_kernel: a full and a part block in the second grid sweep
test_cast_bf16[n] / test_cast_f32[n]         cast_bf16_kernel / cast_f32_kernel: scalar tail only, vector + tail, a tail in the
                                             second sweep
test_axpy[n]                                 axpy_kernel, both ``accumulate`` values, second sweep (2097152 + 300)
test_gather_rows[M-H]                        gather_rows_bf16_kernel, repeated rows, 4100 blocks > the 4096 cap
test_split_bf16[R-rows_out-P]                split_bf16_kernel, both patterns, zero rows, 4104 blocks > the cap
test_dpo_loss[B]                             dpo_loss_kernel: one wave (1, 63, 64), two (65), four (255, 256), a second trip of
                                             the block loop (257, 1000); three modes x three distributions; non-finite batches
test_logits_logprob[V]                       logits_logprob_kernel / logits_logprob_bwd_kernel: V below / at / above one wave
                                             trip, the GPT-2 vocabulary; ld > V; row_map or NULL; R % 4 != 0; four row kinds
test_l2norm[P]                               l2norm_fwd_kernel / l2norm_bwd_kernel: strided loops of 1 .. 16 trips, part block
                                             of rows, zero row, clamped row, norm = NULL
test_ntxent_loss[n_local]                    ntxent_loss_kernel: part wave, four waves, a second trip
test_seq_reduce[nseq]                        seq_reduce_kernel: counts branch (prefix loop of two trips at 70), scan branch
                                             (seq_count = NULL), sum and mean, empty sequences
test_row_scale[nrows]                        row_scale_kernel modes 0-3, part block
test_seq_prepare_and_pack[Bq-S]              seq_counts / seq_compact (ballot loop of 1, 2, 3 trips) / seq_lens / seq_pack
                                             kernels: prefix loops of 1, 2, 3 trips; 1, 4 or 32 filler sequences
test_patchify_past_one_sweep                 patchify_kernel (4263 blocks), patchify_pad_kernel (4160 blocks) > the 4096 cap
test_vit_assemble_past_one_sweep             vit_assemble_kernel (4200 blocks), vit_assemble_bwd_kernel accumulating
===========================================  ==============================================================================

None of these kernels uses atomics: every one is launched twice and the two results (sentinels included) must be bitwise
equal.  Bounds come from step_kernel_refs.py, never from a kernel's output; the one exception is the device's own
``coef[0]``, the multiplier of the bitwise ``scale_dev`` check.  Run with ``-s`` for measured error against bound.
"""
import math

import pytest
import torch

import step_kernel_refs as K
from step_kernel_refs import holds
from test_bench_geometry_gpu import Guard, dev, gen, hip, randn  # noqa: F401  (hip is a fixture)

pytestmark = pytest.mark.gpu

F64 = torch.float64
F32, BF16, I32, I64 = torch.float32, torch.bfloat16, torch.int32, torch.int64
SWEEP4 = K.SWEEP * 4                   # elements of one sweep of the float4 kernels: 8388608
B1, B2, ADAM_EPS, WD = 0.9, 0.999, 1e-8, 0.01
NAN, INF = float("nan"), float("inf")


def flat(n, dtype=F32, fill=None):
    """A flat guarded buffer of exactly n elements (plus sentinel slack behind it)."""
    return Guard(1, n, dtype, pad_rows=0, slack=256, fill=None if fill is None else fill.view(1, n))


def twice(run):
    """Launch twice into fresh buffers: bitwise equal, sentinels included.  ``run`` returns the guards; the first set is
    handed back."""
    a, b = run(), run()
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x.raw, y.raw), f"output {i} differs between two launches"
    return a


def f32t(values):
    return torch.tensor(values, dtype=F32, device=dev())


class IntGuard:
    """Capacity array of an integer kernel output inside a sentinel-filled buffer; ``check`` compares the written prefix
    and requires the sentinel everywhere behind it."""
    SENT = {I32: -0x5A5A5A5B, I64: -0x5A5A5A5A5A5A5A5B}

    def __init__(self, n, dtype=I32, slack=64):
        self.sentinel = self.SENT[dtype]
        self.buf = torch.full((n + slack,), self.sentinel, dtype=dtype, device=dev())

    def check(self, what, want):
        want = torch.tensor(want, dtype=self.buf.dtype)
        got = self.buf.cpu()
        n = want.numel()
        assert torch.equal(got[:n], want), f"{what}: first difference at {int((got[:n] != want).nonzero()[0])}"
        assert bool((got[n:] == self.sentinel).all()), f"{what}: written past its {n} entries"


# =============================================================================================== 1. sqnorm partials
@pytest.mark.parametrize("n", [1, 3, 4, 5, 16383, 16384, 16385, 3 * 16384 + 5])
def test_sqnorm_partials(hip, n):
    nb = (n + K.SQ_BLOCK - 1) // K.SQ_BLOCK
    assert hip.sqnorm_blocks(n) == nb
    for dist in ("normal", "outlier"):
        g = randn((n,), 11 + n)
        if dist == "outlier":
            g[n - 1] = 1e15                          # in the scalar tail / the last slice: dropping either loses 1e30

        def run():
            part = flat(nb)
            hip.sqnorm(g, n, part.view)
            return (part,)
        part, = twice(run)
        part.check(f"sqnorm part n={n}")
        ref, lens = K.sqnorm_ref(g)
        err = (part.view[0].double() - ref).abs()
        holds(f"sqnorm n={n} {dist}", "partials", err, K.sqnorm_bound(ref, lens), "sum_bound(min(16384, len), sum g^2)")
        holds(f"sqnorm n={n} {dist}", f"last partial ({int(lens[-1])} elements)", err[-1:], K.sqnorm_bound(ref, lens)[-1:],
              "sum_bound")


# =============================================================================================== 2. norm from partials
def synthetic_partials(nparts, kind):
    p = 0.5 + torch.rand(nparts, generator=torch.Generator().manual_seed(nparts))
    if kind == "big":
        p[:] = 1.0
        p[nparts // 2] = 2.0 ** 40                   # a float sum loses every 1 next to it; the double sum must not
    elif kind == "nan":
        p[nparts // 3] = NAN
    elif kind == "inf":
        p[nparts - 1] = INF
    return p


@pytest.mark.parametrize("nparts", [1, 255, 256, 257, 1000])
def test_norm_from_partials(hip, nparts):
    for kind in ("unit", "big", "nan", "inf"):
        parts = synthetic_partials(nparts, kind)
        pd = parts.to(dev())
        for gs in (1.0, 0.125, 1.0 / 3.0):
            want = K.norm_from_partials(parts.tolist(), gs)

            def run():
                ctrl, coef = flat(8, fill=torch.zeros(8, device=dev())), flat(2)
                hip.step_control(pd, nparts, 1.0, 5e-5, 3, 8, 2, B1, B2, gs, ctrl.view)
                if gs == 1.0:
                    hip.clip_coef(pd, nparts, 1.0, coef.view)
                return ctrl, coef
            ctrl, coef = twice(run)
            ctrl.check("ctrl")
            coef.check("coef", full=gs == 1.0)
            got = [float(ctrl.view[0, 0])] + ([float(coef.view[0, 1])] if gs == 1.0 else [])
            bound = 2 * float(K.ulp32(want)) if math.isfinite(want) else 0.0
            for name, x in zip(("step_control ctrl[0]", "clip_coef coef[1]"), got):
                assert K.scalar_matches(x, want, bound), f"{name} nparts={nparts} {kind} gs={gs}: {x!r} vs {want!r} +- {bound:.2e}"
            assert float(ctrl.view[0, 1]) == (1.0 if math.isfinite(want) else 0.0)
            if math.isfinite(want):
                K.report(f"norm nparts={nparts} {kind} gs={gs:.3f}", "ctrl[0]", abs(got[0] - want), bound, "2 f32 ulp")


# =============================================================================================== 3. step_control
SC = dict(max_norm=1.0, base_lr=5e-5, warmup=3, total_steps=8, sched_stride=2, beta1=B1, beta2=B2, grad_scale=0.5)
# (partials, gate, max_norm): norm = 0.5 * sqrt(sum)
SEQUENCE = [
    ([1.0, 2.0, 1.0], None, 1.0),          # 1  warm-up, sched 0: lr = 0, norm 1: clip just below 1
    ([0.25, 0.5, 0.25], None, 1.0),        # 2  warm-up, sched 2; norm 0.5: no clipping
    ([30.0, 4.0, 2.0], None, 1.0),         # 3  first cosine step (sched 4 >= warmup 3); norm 3: clip 1/3
    ([1.0, 1.0, 1.0], None, 1.0),          # 4  sched 6
    ([9.0, 0.0, 0.0], None, 1.0),          # 5  sched 8 = total_steps: the end of the schedule, multiplier 0
    ([1.0, 1.0, 2.0], None, 1.0),          # 6  sched 10: prog 1.4, HF's formula turns back up
    ([1.0, 0.5, 0.5], None, 1.0),          # 7  sched 12
    ([0.1, 0.1, 0.1], None, 1.0),          # 8  sched 14: prog 2.2
    ([1.0, NAN, 1.0], None, 1.0),          # 9  NaN partial: skipped
    ([1.0, 1.0, INF], None, 1.0),          # 10 inf partial: skipped
    ([1.0, 1.0, 1.0], NAN, 1.0),           # 11 finite norm, gate NaN: skipped
    ([1.0, 1.0, 1.0], INF, 1.0),           # 12 gate +inf: skipped
    ([1.0, 1.0, 1.0], 0.7, 1.0),           # 13 gate finite: taken (sched 16)
    ([400.0, 0.0, 0.0], None, 0.0),        # 14 max_norm = 0: the clip is exactly 1 whatever the norm
]


def drive(hip, sequence, settings):
    """One ctrl through the sequence; returns the guard and the eight slots (bit patterns too) after every call."""
    ctrl = flat(8, fill=torch.zeros(8, device=dev()))
    snaps = []
    for parts, gate, max_norm in sequence:
        gate_d = None if gate is None else f32t([gate])
        s = dict(settings, max_norm=max_norm)
        hip.step_control(f32t(parts), len(parts), s["max_norm"], s["base_lr"], s["warmup"], s["total_steps"],
                         s["sched_stride"], s["beta1"], s["beta2"], s["grad_scale"], ctrl.view, gate=gate_d)
        torch.cuda.synchronize()
        snaps.append((ctrl.view[0].cpu().double().tolist(), ctrl.view[0].cpu().view(I32).tolist()))
    ctrl.check("ctrl")
    return ctrl, snaps


def check_machine(hip, case, sequence, settings):
    _, snaps = drive(hip, sequence, settings)
    _, again = drive(hip, sequence, settings)
    assert [bits for _, bits in snaps] == [bits for _, bits in again], "two runs of the sequence differ"
    ref, last_bound = [0.0] * 8, [0.0] * 8
    prev_bits = [0] * 8
    worst = 0.0
    for i, ((parts, gate, max_norm), (got, bits)) in enumerate(zip(sequence, snaps), 1):
        ref, bound = K.step_control_ref(ref, parts, **dict(settings, max_norm=max_norm), gate=gate)
        taken = ref[1] == 1.0
        if taken:
            last_bound = bound
        else:
            assert bits[3:] == prev_bits[3:], f"call {i}: a skipped step changed slots 3-7"
            assert got[1] == 0.0
            bound = bound[:3] + last_bound[3:]
        for k in range(8):
            assert K.scalar_matches(got[k], ref[k], bound[k]), \
                f"[{case}] call {i} slot {k}: got {got[k]!r}, reference {ref[k]!r} +- {bound[k]:.3e}"
            if bound[k] > 0 and math.isfinite(ref[k]):
                worst = max(worst, abs(got[k] - ref[k]) / bound[k])
        if max_norm == 0.0:
            assert got[2] == 1.0
        print(f"[{case}] call {i:2d} {'taken  ' if taken else 'skipped'} norm {got[0]:.6g} clip {got[2]:.6g} lr {got[3]:.6e} "
              f"(ref {ref[3]:.6e} +- {bound[3]:.1e}) bc {got[4]:.7f} {got[5]:.7f} step {got[6]:.0f} sched {got[7]:.0f}")
        prev_bits = bits
    print(f"[{case}] worst slot error: {worst:.3f} of its bound")
    return ref


def test_step_control_state_machine(hip):
    assert len(SEQUENCE) == 14
    ref = check_machine(hip, "step_control", SEQUENCE, SC)
    assert ref[6] == 10.0 and ref[7] == 20.0
    # warmup = 0, total_steps = 1: both denominators clamp to 1 (sched 0: lr = base; 1: the end; 2: prog 2, back at base)
    short = [([1.0], None, 1.0)] * 3
    ref = check_machine(hip, "step_control w0 t1", short, dict(SC, warmup=0, total_steps=1, sched_stride=1))
    assert ref[6] == 3.0 and abs(ref[3] - K.r32(5e-5)) < 1e-18


# =============================================================================================== 4. clip_coef + scale_dev
@pytest.mark.parametrize("n", [4, 1028, SWEEP4 + 1088])
def test_clip_coef_and_scale_dev(hip, n):
    x = randn((n,), 21)
    for name, parts in (("below", [0.125, 0.125]), ("above", [9.0, 16.0]), ("nan", [1.0, NAN]), ("inf", [INF, 1.0])):
        pd = f32t(parts)

        def run():
            coef, buf = flat(2), flat(n, fill=x)
            hip.clip_coef(pd, len(parts), 1.0, coef.view)
            hip.scale_dev(buf.view, n, coef.view)
            return coef, buf
        coef, buf = twice(run)
        coef.check("coef")
        buf.check("scaled buffer")
        c0, c1 = float(coef.view[0, 0]), float(coef.view[0, 1])
        norm = K.norm_from_partials(parts)
        if name == "above":
            want = K.R.clip_coefficient(math.sqrt(math.fsum(parts)), 1.0)
            holds(f"clip_coef n={n}", "coef[0]", abs(c0 - want), 2 * float(K.ulp32(want)), "2 ulp of max_norm / (norm + 1e-6)")
            assert c0 < 1.0
            scaled = x * coef.view[0, 0]             # one IEEE multiply by the device's own coefficient: bitwise
            if n > SWEEP4:
                assert torch.equal(buf.view[0, SWEEP4:], scaled[SWEEP4:]), "second grid sweep"
            assert torch.equal(buf.view[0], scaled)
        else:
            assert c0 == 1.0 and coef.view[0, :1].view(I32).item() == 0x3F800000
            assert K.scalar_matches(c1, norm, 2 * float(K.ulp32(norm)) if math.isfinite(norm) else 0.0)
            assert torch.equal(buf.view[0].view(I32), x.view(I32)), f"{name}: the buffer must stay bitwise untouched"


# =============================================================================================== 5. AdamW
def adamw_ctrl(hip, t, lr, clip):
    """ctrl with ctrl[6] = t - 1 set by hand, then one step_control (warmup 0, multiplier 1, no clipping) and the clip
    written by hand: lr is the float lr exactly, the bias corrections are the kernel chain's own powf values."""
    ctrl = torch.zeros(8, device=dev())
    ctrl[6] = float(t - 1)
    hip.step_control(f32t([1.0]), 1, 0.0, lr, 0, 1, 1, B1, B2, 1.0, ctrl)
    ctrl[2] = clip
    c = ctrl.cpu().double().tolist()
    assert c[1] == 1.0 and c[3] == K.r32(lr) and c[6] == float(t)
    return ctrl


def adamw_case(hip, case, n, t, lr, clip, gsc, seed):
    p, g, m, v = K.adamw_state(n, t, gen(seed))
    ctrl = adamw_ctrl(hip, t, lr, clip)

    def run(mirror=True, ctrl=ctrl):
        gp, gm, gv, gb = flat(n, fill=p), flat(n, fill=m), flat(n, fill=v), flat(n, BF16)
        hip.adamw(gp.view, g, gm.view, gv.view, gb.view if mirror else None, n, ctrl, WD, B1, B2, ADAM_EPS, gsc)
        return gp, gm, gv, gb
    gp, gm, gv, gb = twice(run)
    for name, x in (("p", gp), ("m", gm), ("v", gv), ("p_bf16", gb)):
        x.check(f"[{case}] {name}")
    gs = K.r32(K.r32(clip) * K.r32(gsc))
    ref = K.adamw_ref(p.double(), g.double(), m.double(), v.double(), t, K.r32(lr), K.r32(WD), K.r32(B1), K.r32(B2),
                      K.r32(ADAM_EPS), gs)
    got = dict(p=gp.view[0], m=gm.view[0], v=gv.view[0])
    ratios = {}
    for name in "pmv":
        err = (got[name].double() - ref[name]).abs()
        if n > SWEEP4:
            holds(case, f"{name}, second grid sweep", err[SWEEP4:], ref["b" + name][SWEEP4:], "case-5 bound")
        ratios[name] = holds(case, name, err, ref["b" + name], "case-5 bound")
    assert torch.equal(gb.view[0], gp.view[0].bfloat16()), f"[{case}] bf16 mirror"
    # no mirror: the same p, m, v and nothing written to the (unpassed) mirror
    np_, nm, nv, nb = run(mirror=False)
    torch.cuda.synchronize()
    assert torch.equal(np_.raw, gp.raw) and torch.equal(nm.raw, gm.raw) and torch.equal(nv.raw, gv.raw)
    assert bool((nb.raw == nb.sentinel).all())
    # ctrl[1] = 0: nothing changes
    skip = ctrl.clone()
    skip[1] = 0.0
    sp, sm, sv, sb = run(ctrl=skip)
    torch.cuda.synchronize()
    assert torch.equal(sp.view[0].view(I32), p.view(I32)) and torch.equal(sm.view[0].view(I32), m.view(I32))
    assert torch.equal(sv.view[0].view(I32), v.view(I32)) and bool((sb.raw == sb.sentinel).all())
    for x in (sp, sm, sv):
        x.check(f"[{case}] skipped step")
    return ratios


@pytest.mark.parametrize("lr", K.ADAMW_LR)
@pytest.mark.parametrize("t", K.ADAMW_T)
def test_adamw_single_step(hip, t, lr):
    for clip, gsc in ((1.0, 1.0), (0.74, 0.5)):      # clip * grad_scale = 1 and 0.37 (the f32 product is exact)
        adamw_case(hip, f"adamw t={t} lr={lr:g} gs={clip * gsc:.2f}", 4096, t, lr, clip, gsc, seed=100 + t)


def test_adamw_second_sweep(hip):
    adamw_case(hip, "adamw n=8388608+1088 t=10", SWEEP4 + 1088, 10, 1e-2, 0.74, 0.5, seed=7)


# =============================================================================================== 6. casts, axpy, gather, split
@pytest.mark.parametrize("n", [1, 3, 1000, SWEEP4 + 1027])
def test_cast_bf16(hip, n):
    x = randn((n,), 31)

    def run():
        y = flat(n, BF16)
        hip.cast_bf16(x, y.view, n)
        return (y,)
    y, = twice(run)
    y.check(f"cast_bf16 n={n}")
    if n > SWEEP4:
        assert torch.equal(y.view[0, SWEEP4:], x[SWEEP4:].bfloat16()), "second grid sweep (scalar tail included)"
    assert torch.equal(y.view[0], x.bfloat16())


@pytest.mark.parametrize("n", [1, 7, 8, 9, 1003, K.SWEEP * 8 + 2051])
def test_cast_f32(hip, n):
    x = randn((n,), 32, dtype=BF16)

    def run():
        y = flat(n)
        hip.cast_f32(x, y.view, n)
        return (y,)
    y, = twice(run)
    y.check(f"cast_f32 n={n}")
    if n > K.SWEEP * 8:
        assert torch.equal(y.view[0, K.SWEEP * 8:], x[K.SWEEP * 8:].float()), "second grid sweep (scalar tail included)"
    assert torch.equal(y.view[0], x.float())


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("n", [1, 257, K.SWEEP + 300])
def test_axpy(hip, n, accumulate):
    x, y0, alpha = randn((n,), 33), randn((n,), 34), 0.37

    def run():
        y = flat(n, fill=y0)
        hip.axpy(x, alpha, y.view, n, accumulate=accumulate)
        return (y,)
    y, = twice(run)
    y.check(f"axpy n={n}")
    ax = K.r32(alpha) * x.double()
    ref = y0.double() + ax if accumulate else ax
    bound = 2 * K.EPS * ((y0.double().abs() if accumulate else 0.0) + ax.abs())
    err = (y.view[0].double() - ref).abs()
    if n > K.SWEEP:
        holds(f"axpy n={n} acc={accumulate}", "second grid sweep", err[K.SWEEP:], bound[K.SWEEP:], "2 eps (|y| + |a x|)")
    holds(f"axpy n={n} acc={accumulate}", "y", err, bound, "2 eps (|y| + |a x|)")


@pytest.mark.parametrize("M,H", [(4, 8), (37, 72), (8200, 1024)])
def test_gather_rows(hip, M, H):
    src = randn((1000, H), 35, dtype=BF16)
    rmap = torch.randint(0, 1000, (M,), generator=gen(M), device=dev(), dtype=I32)
    rmap[0], rmap[1], rmap[M - 1] = 999, 999, 0

    def run():
        dst = Guard(M, H, BF16)
        hip.gather_rows_bf16(src, rmap, M, H, dst.view)
        return (dst,)
    dst, = twice(run)
    dst.check(f"gather {M}x{H}")
    assert torch.equal(dst.view, src[rmap.long()])


@pytest.mark.parametrize("R_,rows_out,P", [(1, 1, 8), (5, 8, 72), (4100, 4104, 1024)])
def test_split_bf16(hip, R_, rows_out, P):
    x = K.split_inputs(R_, P, gen(36))
    for pattern in (0, 1):
        def run():
            y = Guard(rows_out, 3 * P, BF16)
            hip.split_bf16(x, R_, P, rows_out, pattern, y.view)
            return (y,)
        y, = twice(run)
        y.check(f"split {R_}x{P} pattern {pattern}")
        ref = K.split_ref(x, rows_out, pattern)
        assert torch.equal(y.view.view(torch.int16), ref.view(torch.int16)), f"pattern {pattern}"
        assert not bool(y.view[R_:].any())


# =============================================================================================== 7. dpo_loss
def dpo_launch(hip, pw, pl, rw, rl, B, ls):
    def run():
        loss, dw, dl, met = flat(1), flat(B), flat(B), flat(4)
        hip.dpo_loss(pw, pl, rw, rl, B, 0.1, ls, loss.view, dw.view, dl.view, met.view)
        return loss, dw, dl, met
    out = twice(run)
    for name, x in zip(("loss", "dpol_w", "dpol_l", "metrics"), out):
        x.check(f"dpo {name}")
    return out


@pytest.mark.parametrize("B", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_dpo_loss(hip, B):
    names = ("reward_margin", "reward_accuracy", "mean pol_w", "mean pol_l")
    for dist in ("workload", "saturating", "ties"):
        pw, pl, rw, rl = K.dpo_inputs(B, dist, gen(B))
        for mode, ls, use_ref in (("ref", 0.0, True), ("ref+ls", 0.1, True), ("ref-free", 0.0, False)):
            case = f"dpo B={B} {dist} {mode}"
            a, b = (rw, rl) if use_ref else (None, None)
            loss, dw, dl, met = dpo_launch(hip, pw, pl, a, b, B, ls)
            ref = K.dpo_ref(pw, pl, a, b, K.r32(0.1), K.r32(ls))
            assert ref["finite"]
            holds(case, "loss", abs(float(loss.view[0, 0]) - ref["loss"]), ref["b_loss"], "sum_bound / B + 1e-5 max(1, |loss|)")
            for k in range(4):
                holds(case, names[k], abs(float(met.view[0, k]) - ref["metrics"][k]), ref["b_metrics"][k],
                      "sum_bound / B + 1e-5 max(1, |mean|)")
            for name, got, want in (("dpol_w", dw, ref["dpw"]), ("dpol_l", dl, ref["dpl"])):
                assert bool(torch.isfinite(got.view).all()), f"[{case}] {name} is not finite"
                holds(case, name, (got.view[0].double() - want).abs(), 1e-4 * want.abs() + 1e-7 * 8.0 / B,
                      "rtol 1e-4, atol 1e-7 * 8 / B")
            if dist == "ties" and use_ref:
                assert ref["metrics"][1] == 0.0 and float(met.view[0, 1]) == 0.0, "ties: the comparison is strict"
    # non-finite batches: the loss is non-finite as in the reference, every gradient seed is exactly zero
    for kind in ("nan", "inf-inf"):
        pw, pl, rw, rl = K.dpo_inputs(B, "workload", gen(B + 5000))
        if kind == "nan":
            pw[B // 2] = NAN
        else:
            pw[B - 1], pl[B - 1] = -INF, -INF
        loss, dw, dl, _ = dpo_launch(hip, pw, pl, rw, rl, B, 0.0)
        assert not K.dpo_ref(pw, pl, rw, rl, K.r32(0.1), 0.0)["finite"]
        assert not math.isfinite(float(loss.view[0, 0])), f"dpo B={B} {kind}: loss"
        assert bool((dw.view == 0).all()) and bool((dl.view == 0).all()), f"dpo B={B} {kind}: gradient seeds must be zero"


# =============================================================================================== 8. logits log-prob
N_LOGIT_ROWS = 64


@pytest.mark.parametrize("V", [1, 63, 64, 65, 1000, 50257])
def test_logits_logprob(hip, V):
    ld = V + 24
    g0 = gen(V)
    perm = torch.randperm(N_LOGIT_ROWS - 3, generator=g0, device=dev()) + 3         # never rows 0 and 2 first (below)
    tgt_of_row = torch.randint(0, V, (N_LOGIT_ROWS,), generator=g0, device=dev())
    for rows in (perm, torch.arange(N_LOGIT_ROWS, device=dev())):       # targets 0 and V - 1 among the first scored rows
        tgt_of_row[rows[0]], tgt_of_row[rows[2]] = 0, V - 1
    rows32 = K.logit_rows(N_LOGIT_ROWS, V, tgt_of_row.tolist(), g0)
    logits = torch.full((N_LOGIT_ROWS, ld), 3e38, device=dev())          # a read past V makes the lse visibly wrong
    logits[:, :V] = rows32
    rows64 = rows32.double()
    zeros = torch.zeros(N_LOGIT_ROWS, V, device=dev())
    worst_f = worst_b = 0.0
    for R_ in (1, 4, 5, 37):
        for use_map in (True, False):
            case = f"logprob V={V} R={R_} {'row_map' if use_map else 'NULL map'}"
            scored = perm[:R_] if use_map else torch.arange(R_, device=dev())
            rmap = scored.to(I32) if use_map else None
            tgt = tgt_of_row[scored].contiguous()
            g = randn((R_,), V + R_)
            g[0] = 0.0
            if R_ > 1:
                g[1] = -0.5 - g[1].abs()

            def run():
                out = flat(R_)
                dl = Guard(N_LOGIT_ROWS, V, F32, ld=ld, fill=zeros)
                hip.logits_logprob(logits, ld, V, rmap, tgt, R_, out.view)
                hip.logits_logprob_bwd(logits, ld, V, rmap, tgt, g, R_, dl.view)
                return out, dl
            out, dl = twice(run)
            out.check(f"[{case}] out")
            dl.check(f"[{case}] dlogits")
            lp, b_lp = K.logprob_ref(rows64[scored], tgt)
            worst_f = max(worst_f, holds(case, "log-prob", (out.view[0].double() - lp).abs(), b_lp,
                                         "4 eps23 (1 + ln V + |max| + |lse| + |x_t|)"))
            dref, b_d = K.logprob_bwd_ref(rows64[scored], tgt, g.double())
            full_ref = torch.zeros(N_LOGIT_ROWS, V, dtype=F64, device=dev())
            full_b = torch.zeros_like(full_ref)
            full_ref[scored], full_b[scored] = dref, b_d
            worst_b = max(worst_b, holds(case, "dlogits (unscored rows must stay zero)", (dl.view.double() - full_ref).abs(),
                                         full_b, "per-element backward bound (+ the f32 underflow floor)"))
    print(f"[logprob V={V}] worst ratio: forward {worst_f:.3f}, backward {worst_b:.3f}")
    # R = 0: returns OK and writes nothing
    dl = Guard(N_LOGIT_ROWS, V, F32, ld=ld, fill=zeros)
    hip.logits_logprob_bwd(logits, ld, V, None, tgt_of_row, randn((1,), 1), 0, dl.view)
    torch.cuda.synchronize()
    dl.check("R = 0")
    assert not bool(dl.view.any())


# =============================================================================================== 9. l2norm
@pytest.mark.parametrize("P", [1, 63, 64, 65, 256, 1000])
def test_l2norm(hip, P):
    for B in (1, 4, 5, 33):
        case = f"l2norm B={B} P={P}"
        x = K.l2norm_rows(B, P, gen(B * 1000 + P))
        dy = randn((B, P), B + P)
        ref = K.l2norm_ref(x, dy)
        y_in, n_in = ref["y"].float().contiguous(), ref["norm"].float().contiguous()   # the backward's inputs: rounded reference

        def run():
            y, n, dx, y2 = Guard(B, P, F32), flat(B), Guard(B, P, F32), Guard(B, P, F32)
            hip.l2norm_fwd(x, B, P, y.view, n.view)
            hip.l2norm_fwd(x, B, P, y2.view, None)
            hip.l2norm_bwd(dy, y_in, n_in, B, P, dx.view)
            return y, n, dx, y2
        y, n, dx, y2 = twice(run)
        for name, o in (("y", y), ("norm", n), ("dx", dx), ("y (norm = NULL)", y2)):
            o.check(f"[{case}] {name}")
        assert torch.equal(y.raw, y2.raw), "norm = NULL changes y"
        holds(case, "y", (y.view.double() - ref["y"]).abs(), ref["by"], "|y| (sum_bound / 2 sum x^2 + 3 eps)")
        holds(case, "norm", (n.view[0].double() - ref["norm"]).abs(), ref["bn"], "n (sum_bound / 2 sum x^2 + 2 eps); clamped: exact")
        holds(case, "dx", (dx.view.double() - ref["dx"]).abs(), ref["bdx"], "sum_bound of dy.y through the quotient")


# =============================================================================================== 10. ntxent_loss
@pytest.mark.parametrize("n_local", [1, 255, 256, 257, 1000])
def test_ntxent_loss(hip, n_local):
    lr, lc, dg = randn((n_local,), 41) + 5.0, randn((n_local,), 42) + 5.0, randn((n_local,), 43) + 3.0
    for n_total in (n_local, 2 * n_local):
        def run():
            loss = flat(1)
            hip.ntxent_loss(lr, lc, dg, n_local, n_total, loss.view)
            return (loss,)
        loss, = twice(run)
        loss.check("ntxent loss")
        want, bound = K.ntxent_ref(lr, lc, dg, n_total)
        holds(f"ntxent n_local={n_local} n_total={n_total}", "loss", abs(float(loss.view[0, 0]) - want), bound,
              "sum_bound(2 n_local, sum |terms|) / (2 n_total)")


# =============================================================================================== 11. seq_reduce / row_scale
SEQ_COUNTS = {1: [200], 4: [64, 0, 65, 1], 5: [0, 1, 64, 65, 200], 70: [[3, 0, 1, 64, 65, 200, 17][i % 7] for i in range(70)]}


@pytest.mark.parametrize("nseq", [1, 4, 5, 70])
def test_seq_reduce(hip, nseq):
    counts = torch.tensor(SEQ_COUNTS[nseq], dtype=I32, device=dev())
    nrows = int(counts.sum())
    seq_of_row = torch.repeat_interleave(torch.arange(nseq, device=dev()), counts.long()).to(I32)
    tok = randn((nrows,), 50 + nseq) - 3.0
    for name, mode, cnt in (("sum, counts", 0, counts), ("mean, counts", 1, counts), ("sum, scan (seq_count = NULL)", 0, None)):
        def run():
            out = flat(nseq)
            hip.seq_reduce(tok, seq_of_row, nrows, nseq, cnt, mode, out.view)
            return (out,)
        out, = twice(run)
        out.check(f"seq_reduce {name}")
        ref, bound = K.seq_reduce_ref(tok, counts, mode)
        got = out.view[0].double()
        live = counts > 0 if mode else torch.ones_like(counts, dtype=torch.bool)
        if mode:
            assert bool(torch.isnan(got[~live]).all()) and bool(torch.isnan(ref[~live]).all()), "mean of an empty sequence is NaN"
        holds(f"seq_reduce nseq={nseq}", name, (got[live] - ref[live]).abs(), bound[live], "sum_bound(count, sum |tok|)")


@pytest.mark.parametrize("nrows", [1, 256, 257, 1000])
def test_row_scale(hip, nrows):
    nseq = 7
    seq_of_row = torch.randint(0, nseq, (nrows,), generator=gen(nrows), device=dev()).sort().values.to(I32)
    counts = torch.bincount(seq_of_row.long(), minlength=nseq).to(I32)
    dseq = randn((nseq,), 60)
    for mode in (0, 1, 2, 3):
        def run():
            rs = flat(nrows)
            hip.row_scale(dseq, seq_of_row, counts, nrows, mode, rs.view)
            return (rs,)
        rs, = twice(run)
        rs.check(f"row_scale mode {mode}")
        ref = K.row_scale_ref(dseq, seq_of_row, counts, mode)
        if mode & 1:
            holds(f"row_scale nrows={nrows}", f"mode {mode}", (rs.view[0].double() - ref).abs(), K.ulp32(ref), "one division's ulp")
        else:
            assert torch.equal(rs.view[0].double(), ref), f"mode {mode} is a copy"


# =============================================================================================== 12. index builders
def prepare_and_pack(hip, ids, mask):
    Bq, S = ids.shape
    F_ = (63 + S - 1) // S
    cap, cap_pack = Bq * (S - 1), (Bq * S + 63) // 64 * 64
    ids_d, mask_d = ids.to(dev()), mask.to(dev())
    o = dict(counts=IntGuard(Bq), mask32=IntGuard((Bq + F_) * S), row_map=IntGuard(cap), targets=IntGuard(cap, I64),
             seq_of_row=IntGuard(cap), n_rows=IntGuard(1))
    hip.seq_batch_prepare(ids_d, mask_d, Bq, S, o["counts"].buf, o["mask32"].buf, o["row_map"].buf, o["targets"].buf,
                          o["seq_of_row"].buf, o["n_rows"].buf)
    torch.cuda.synchronize()
    packs = []
    for with_map in (True, False):
        pk = dict(lens=IntGuard(Bq), cu=IntGuard(Bq + F_ + 1), row_ids=IntGuard(cap_pack), n_packed=IntGuard(2),
                  mask32=IntGuard((Bq + F_) * S), row_map=IntGuard(cap))
        pk["mask32"].buf.copy_(o["mask32"].buf)
        pk["row_map"].buf.copy_(o["row_map"].buf)
        hip.seq_pack_prepare(pk["mask32"].buf, Bq, S, 64, pk["lens"].buf, pk["cu"].buf, pk["row_ids"].buf,
                             pk["n_packed"].buf, counts=o["counts"].buf if with_map else None,
                             row_map=pk["row_map"].buf if with_map else None)
        packs.append(pk)
    torch.cuda.synchronize()
    return o, packs


INDEX_CASES = [(Bq, S, False) for Bq in (1, 65, 130) for S in (2, 64, 65, 66, 129)] + \
              [(5, 16, False), (4, 64, True), (8, 16, True)]


@pytest.mark.parametrize("Bq,S,full", INDEX_CASES)
def test_seq_prepare_and_pack(hip, Bq, S, full):
    ids, mask = K.index_batch(Bq, S, torch.Generator().manual_seed(Bq * 1000 + S), full=full)
    o, packs = prepare_and_pack(hip, ids, mask)
    o2, packs2 = prepare_and_pack(hip, ids, mask)
    for a, b in [(o, o2)] + list(zip(packs, packs2)):
        for k in a:
            assert torch.equal(a[k].buf, b[k].buf), f"{k} differs between two launches"
    ref = K.seq_batch_prepare_ref(ids.tolist(), mask.tolist())
    flat_mask = [x for row in ref["mask32"] for x in row]
    o["counts"].check("counts", ref["counts"])
    o["row_map"].check("row_map", ref["row_map"])
    o["targets"].check("targets (int64, bit-exact)", ref["targets"])
    o["seq_of_row"].check("seq_of_row", ref["seq_of_row"])
    o["n_rows"].check("n_rows", [ref["n"]])
    o["mask32"].check("mask32", flat_mask)
    assert int(ids.max()) > 1 << 32 and (full or S == 2 or int(mask.min()) == -1)
    for pk, with_map in zip(packs, (True, False)):
        want = K.seq_pack_prepare_ref(ref["mask32"], S, 64, ref["counts"] if with_map else None,
                                      ref["row_map"] if with_map else None)
        assert want["F"] == (1 if S >= 63 else -(-63 // S))
        pk["lens"].check("lens", want["lens"])
        pk["cu"].check("cu", want["cu"])
        pk["row_ids"].check("row_ids", want["row_ids"])
        pk["n_packed"].check("n_packed", [want["n"], want["padded"]])
        pk["mask32"].check("mask32 + filler rows", flat_mask + [1] * (want["F"] * S))
        pk["row_map"].check("row_map (packed)" if with_map else "row_map (not passed: untouched)",
                            want["row_map"] if with_map else ref["row_map"])
    if full:
        assert want["n"] == want["padded"] == Bq * S, "a packed length that is already a multiple of 64: no filler row"


# =============================================================================================== 13. ViT input kernels
@pytest.mark.parametrize("B,I,P,ld", [(29, 224, 32, 3072), (13, 224, 14, 640)])
def test_patchify_past_one_sweep(hip, B, I, P, ld):
    px = randn((B, 3, I, I), 70)
    G = I // P

    def run():
        out = Guard(B * G * G, ld, BF16)
        hip.patchify(px, B, I, P, out.view, ld_out=ld)
        return (out,)
    out, = twice(run)
    out.check(f"patchify P={P}")
    ref = K.patchify_ref(px, P, ld)
    assert torch.equal(out.view[:, 3 * P * P:], ref[:, 3 * P * P:]) and not bool(ref[:, 3 * P * P:].any()), "pad columns"
    assert torch.equal(out.view, ref)


def test_vit_assemble_past_one_sweep(hip):
    B, T, H = 28, 50, 768
    pe, cls, pos = randn((B * (T - 1), H), 71), randn((H,), 72), randn((T, H), 73)

    def run():
        x = Guard(B * T, H, F32)
        hip.vit_assemble(pe, cls, pos, B, T, H, x.view)
        return (x,)
    x, = twice(run)
    x.check("vit_assemble")
    assert torch.equal(x.view.view(B, T, H), K.vit_assemble_ref(pe, cls, pos, B, T, H))


@pytest.mark.parametrize("B", [3, 28])
def test_vit_assemble_bwd_accumulates(hip, B):
    T, H = 50, 768
    dx = randn((B, T, H), 74)
    dcls0, dpos0 = randn((H,), 75, 0.1), randn((T, H), 76, 0.1)          # non-zero: the kernel accumulates onto them

    def run():
        dp, dc, dq = Guard(B * (T - 1), H, BF16), flat(H, fill=dcls0), Guard(T, H, F32, fill=dpos0)
        hip.vit_assemble_bwd(dx, B, T, H, dp.view, dc.view, dq.view)
        return dp, dc, dq
    dp, dc, dq = twice(run)
    for name, o in (("dpatch", dp), ("dcls", dc), ("dpos", dq)):
        o.check(f"vit_assemble_bwd {name}")
    ref = K.vit_assemble_bwd_ref(dx, dcls0, dpos0)
    assert torch.equal(dp.view.double(), ref["dpatch"]), "dpatch is the exact bf16 of dx"
    holds(f"vit_assemble_bwd B={B}", "dpos", (dq.view.double() - ref["dpos"]).abs(), ref["b_dpos"], "sum_bound(B, sum |dx|)")
    holds(f"vit_assemble_bwd B={B}", "dcls", (dc.view[0].double() - ref["dcls"]).abs(), ref["b_dcls"], "sum_bound(B, sum |dx|)")
