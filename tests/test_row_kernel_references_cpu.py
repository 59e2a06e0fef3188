"""The float64 references of ``test_bench_geometry_rows_gpu.py`` (tests/row_kernel_refs.py) against ``torch.autograd`` at
tiny sizes, so that a reference cannot be wrong in the way a kernel is; plus the CPU-side properties the GPU module
relies on: the sharp attention inputs have a finite lse and no probability row that underflows in float32, and the
LayerNorm stress rows are (or are not) within reach of a correctly rounded float32 two-pass computation."""
import pytest
import torch

import row_kernel_refs as K
from oracle import restatement as R

F64 = torch.float64


def test_drop_mult_at_is_the_oracle_hash():
    n = 5000
    want = R.dropout_multiplier(0xC0FFEE, 0.1, n).double()
    got = K.drop_mult_at(0xC0FFEE, 0.1, torch.arange(n))
    assert torch.equal(got, want)
    got = K.drop_mult_at(77, 0.3, torch.arange(1000, n))             # an offset window, as the chunked references use it
    assert torch.equal(got, R.dropout_multiplier(77, 0.3, n).double()[1000:])
    # indices wrap modulo 2^32 like the kernels' unsigned arithmetic (filler rows: drop_rows = -1)
    assert torch.equal(K.drop_mult_at(5, 0.1, torch.tensor([-1 * 8 + 3])),
                       K.drop_mult_at(5, 0.1, torch.tensor([(1 << 32) - 8 + 3])))


def _attn_case(seed, nb=3, S=12, heads=2, holes=False):
    g = torch.Generator().manual_seed(seed)
    q, k, v, dout = (torch.randn(nb, heads, S, 64, generator=g, dtype=F64) for _ in range(4))
    lens = torch.tensor([S, 5, 1][:nb])
    mask = (torch.arange(S)[None] < lens[:, None]).int()
    if holes:
        mask[0, 3] = 0
        mask[1, 0] = 0                                               # query 0 of sequence 1 has NO allowed key
    mult = K.attn_drop_mult(99, 0.25, 0, nb, heads, S, "cpu")
    return q, k, v, dout, mask, mult


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("drop", [False, True])
def test_attention_backward_formula_is_autograd(causal, drop):
    q, k, v, dout, mask, mult = _attn_case(1)
    if not drop:
        mult = None
    S = q.shape[2]
    allowed = K.attn_allowed(mask, S, causal)
    if not causal:   # (without the causal edge a padded key would leave no row empty, but keep every row non-empty)
        allowed = K.attn_allowed(torch.ones_like(mask), S, causal)
    qa, ka, va = (t.clone().requires_grad_() for t in (q, k, v))
    s = (qa @ ka.transpose(-1, -2)) * 0.125
    p = torch.softmax(s.masked_fill(~allowed, float("-inf")), -1)
    ref = (p if mult is None else p * mult) @ va
    ref.backward(dout)
    out, lse, P = K.attn_fwd_ref(q, k, v, allowed, mult)
    assert torch.allclose(out, ref.detach(), rtol=1e-12, atol=1e-13)
    assert torch.allclose(lse, torch.logsumexp(s.detach().masked_fill(~allowed, float("-inf")), -1), rtol=1e-12, atol=1e-13)
    dq, dk, dv = K.attn_bwd_ref(q, k, v, dout, allowed, mult)
    for a, b in ((dq, qa.grad), (dk, ka.grad), (dv, va.grad)):
        assert torch.allclose(a, b, rtol=1e-11, atol=1e-12)


def test_attention_row_without_an_allowed_key():
    """key_mask zero at position 0: the causal query 0 sees nothing.  The reference pins out = 0, lse = -inf and no
    gradient through that row (autograd of the same graph with that row's probabilities replaced by zeros)."""
    q, k, v, dout, mask, mult = _attn_case(2, holes=True)
    S = q.shape[2]
    allowed = K.attn_allowed(mask, S, True)
    empty = ~allowed.any(-1)                                          # [b, 1, S]
    assert bool(empty[1, 0, 0]) and int(empty.sum()) == 1
    out, lse, P = K.attn_fwd_ref(q, k, v, allowed, mult)
    assert torch.isfinite(out).all() and float(out[1, :, 0].abs().max()) == 0.0
    assert bool(torch.isinf(lse[1, :, 0]).all()) and bool((lse[1, :, 0] < 0).all())
    assert int(torch.isinf(lse).sum()) == lse.shape[1]
    qa, ka, va = (t.clone().requires_grad_() for t in (q, k, v))
    s = (qa @ ka.transpose(-1, -2)) * 0.125
    al2 = allowed | empty[..., None]                                  # give the empty row every key, then zero its P
    p = torch.softmax(s.masked_fill(~al2, float("-inf")), -1) * (~empty[..., None]).double()
    ((p * mult) @ va).backward(dout)
    dq, dk, dv = K.attn_bwd_ref(q, k, v, dout, allowed, mult)
    for a, b in ((dq, qa.grad), (dk, ka.grad), (dv, va.grad)):
        assert torch.isfinite(a).all() and torch.allclose(a, b, rtol=1e-11, atol=1e-12)
    assert float(dq[1, :, 0].abs().max()) == 0.0
    # the emulation with the kernels' rounding points handles the row the same way
    eo, edq, edk, edv = K.attn_emulated(q, k, v, dout, allowed, mult)
    assert all(bool(torch.isfinite(t).all()) for t in (eo, edq, edk, edv))
    assert float(eo[1, :, 0].abs().max()) == 0.0 and float(edq[1, :, 0].abs().max()) == 0.0


def test_attention_emulation_is_close_to_float64_and_not_equal():
    q, k, v, dout, mask, mult = _attn_case(3)
    q, k, v, dout = (K.bf16_round(t) for t in (q, k, v, dout))
    allowed = K.attn_allowed(mask, q.shape[2], True)
    out, _, _ = K.attn_fwd_ref(q, k, v, allowed, mult)
    grads = K.attn_bwd_ref(q, k, v, dout, allowed, mult)
    emu = K.attn_emulated(q, k, v, dout, allowed, mult)
    for a, b in zip(emu, (out,) + grads):
        err = float((a - b).abs().max() / b.abs().max())
        assert 0.0 < err < 2.0 ** -6, err                             # a few bf16 roundings, not zero and not garbage


def test_sharp_inputs_have_finite_lse_and_no_underflowed_row():
    nb, S, heads = 4, 128, 3
    g = torch.Generator().manual_seed(4)
    x = K.sharp_qkv(nb, S, heads, g, shift_head=1).bfloat16()
    q, k, v = (K.split_heads(x[:, i * heads * 64:(i + 1) * heads * 64], nb, S, heads) for i in range(3))
    lens = torch.tensor([128, 65, 17, 1])
    mask = (torch.arange(S)[None] < lens[:, None]).int()
    allowed = K.attn_allowed(mask, S, True)
    s = (q @ k.transpose(-1, -2)) * 0.125
    sd = float(s[0, 0][:, 1:][torch.tril(torch.ones(S, S, dtype=torch.bool))[:, 1:]].std())
    assert 7.0 < sd < 9.0, sd                                         # scores have standard deviation ~ 8
    assert 50.0 < float((s[:, 0, :, 0] - 0).mean()) < 70.0            # the sink: about +60 for every query
    assert -84.0 < float(s[:, 1][allowed[:, 0].expand_as(s[:, 1])].mean()) < -76.0   # the shifted head: every score about -80
    _, lse, P = K.attn_fwd_ref(q, k, v, allowed)
    rows = (torch.arange(S)[None] < lens[:, None])[:, None, :].expand_as(lse)
    assert bool(torch.isfinite(lse[rows]).all())
    # float32 with the maximum subtracted: no row of exp(s - max) sums to zero ...
    s32 = s.float().masked_fill(~allowed, float("-inf"))
    e32 = torch.exp(s32 - s32.amax(-1, keepdim=True))
    assert float(e32.sum(-1)[rows].min()) >= 1.0
    # ... while WITHOUT the subtraction float32 does not survive them: every row of the shifted head sums to less than
    # 1e-15, some to less than the smallest normal float32 (1.2e-38), and the sink of the other heads overflows exp()
    # wherever 60 + N(0, 8) exceeds 88.7 - so a kernel that skips the subtraction cannot pass
    naive = torch.exp(s.masked_fill(~allowed, float("-inf")))[:, 1].sum(-1)[rows[:, 1]]
    assert float(naive.max()) < 1e-15 and float(naive.min()) < 1.2e-38


@pytest.mark.parametrize("H", [64, 1600])
def test_layernorm_backward_formula_is_autograd(H):
    M = 7
    g = torch.Generator().manual_seed(H)
    x, dy, add = (torch.randn(M, H, generator=g, dtype=F64) for _ in range(3))
    gamma, beta = torch.randn(H, generator=g, dtype=F64) * 0.1 + 1, torch.randn(H, generator=g, dtype=F64)
    m_add = K.drop_mult_at(1, 0.1, torch.arange(M * H)).view(M, H)
    m_dx = K.drop_mult_at(2, 0.1, torch.arange(M * H)).view(M, H)
    xa, ga, ba = x.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    y = torch.nn.functional.layer_norm(xa, (H,), ga, ba, 1e-5)
    yr, mean, rstd = K.ln_fwd_ref(x, gamma, beta)
    assert torch.allclose(yr, y.detach(), rtol=1e-12, atol=1e-13)
    y.backward(dy)
    dx_out, dxb, planes = K.ln_bwd_full_ref(x, gamma, dy, add, m_add, m_dx)
    assert torch.allclose(dx_out, xa.grad + add, rtol=1e-10, atol=1e-12)
    assert torch.allclose(dxb, (xa.grad + add) * m_dx, rtol=1e-10, atol=1e-12)
    assert torch.allclose(planes[0].sum(0), ga.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(planes[1].sum(0), ba.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(planes[2].sum(0), (add * m_add).sum(0), rtol=1e-12)
    assert torch.allclose(planes[3].sum(0), ((xa.grad + add) * m_dx).sum(0), rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("xheads,shared", [(0, False), (4, True)])
def test_embedding_composite_backward_is_autograd(xheads, shared):
    B, S, H, V = 3, 6, 32, 11
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(0, V, (B, S), generator=g)
    ids[0, :3] = 7
    wte, wpe = torch.randn(V, H, generator=g, dtype=F64), torch.randn(S + 2, H, generator=g, dtype=F64)
    att = torch.randn(H, generator=g, dtype=F64) if shared else torch.randn(B, H, generator=g, dtype=F64)
    U = torch.randn(B, xheads, H, generator=g, dtype=F64) if xheads else None
    w = K.drop_mult_at(3, 0.3, torch.arange(B * xheads * S)).view(B, xheads, S) if xheads else None
    me = K.drop_mult_at(4, 0.1, torch.arange(B * S * H)).view(B, S, H) if xheads else None
    gamma, beta = torch.randn(H, generator=g, dtype=F64) * 0.1 + 1, torch.randn(H, generator=g, dtype=F64)
    rmask = torch.ones(B, S, dtype=torch.int32)
    rmask[1, 4:] = 0
    gout = torch.randn(B, S, H, generator=g, dtype=F64)
    leaves = [t.clone().requires_grad_() for t in (wte, wpe, att, gamma, beta)] + ([U.clone().requires_grad_()] if xheads else [])
    wa, pa, aa, ga, ba = leaves[:5]
    Ua = leaves[5] if xheads else None
    e = wa[ids] + (aa[None, None] if shared else aa[:, None])
    if xheads:
        e = e + torch.einsum("bhs,bhc->bsc", w, Ua)
    h0 = torch.nn.functional.layer_norm(e, (H,), ga, ba, 1e-5) + pa[:S][None]
    if me is not None:
        h0 = h0 * me
    h0r, er = K.embed_fwd_ref(ids, wte, wpe, att, U, w, gamma, beta, me)
    assert torch.allclose(h0r, h0.detach(), rtol=1e-12, atol=1e-13)
    h0.backward(gout * rmask[..., None])
    r = K.embed_bwd_ref(gout, ids, rmask, er, U, w, gamma, me, V)
    assert torch.allclose(r["dwte"], wa.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(r["dwpe"], pa.grad[:S], rtol=1e-10, atol=1e-12)
    assert torch.allclose(r["datt"].sum(0) if shared else r["datt"], aa.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(r["dgamma"], ga.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(r["dbeta"], ba.grad, rtol=1e-10, atol=1e-12)
    if xheads:
        assert torch.allclose(r["dU"], Ua.grad, rtol=1e-10, atol=1e-12)
    assert bool((r["abs_dwte"] >= r["dwte"].abs() - 1e-12).all())
    assert float(r["n_dwte"].sum()) == float(rmask.sum())


@pytest.mark.parametrize("H", [1024, 1280, 1600])
def test_layernorm_stress_rows_against_a_rounded_f32_two_pass(H):
    """Which stress rows a correctly rounded float32 two-pass LayerNorm carries within the per-row bounds of the GPU test
    (y 1e-5, the dx gradient 2e-5 of the row scale): decided HERE, from float64, not from the kernel.
    The constant row passes (3.25 * H is exact in f32 in any summation order, so mean is exact, the variance exactly 0 and
    y = beta); the mean-1e3 row does not: x - mean carries the 2^-24 * 1e3 = 6e-5 rounding of the f32 mean against values of
    order 1.  The GPU module therefore keeps all three in the forward test (the mean-1e3 row measured, reported and held to
    the rounding of its f32 mean) and only ``LN_GRAD_STRESS`` in the gradient checks."""
    g = torch.Generator().manual_seed(H)
    x = K.ln_stress_rows(H, g)
    gamma, beta = torch.randn(H, generator=g) * 0.1 + 1, torch.randn(H, generator=g) * 0.1
    y64, mean64, rstd64 = K.ln_fwd_ref(x.double(), gamma.double(), beta.double())
    y32, mean32, rstd32 = K.f32_two_pass_ln(x, gamma, beta)
    assert abs(float(rstd64[0]) - 1e-5 ** -0.5) < 1e-9                # variance exactly 0
    assert bool(torch.isfinite(y32).all())
    ok = {}
    for i, name in enumerate(K.LN_STRESS):
        scale = float(y64[i].abs().max()) + 1e-30
        err = float((y32[i].double() - y64[i]).abs().max())
        ok[name] = err <= 0.5e-5 * scale and abs(float(rstd32[i]) - float(rstd64[i])) <= 0.5e-5 * float(rstd64[i])
        # every stress row stays within the bound the GPU forward test holds it to (row bound + the f32 rounding of x - mean)
        assert err <= float(K.ln_stress_fwd_bound(x[i].double(), gamma.double(), y64[i], rstd64[i])), (name, err)
    # a row enters the gradient checks only if the rounded f32 computation meets the 1e-5 bound with a factor 2 to spare
    # at every H (the mean-1e3 row sits AT the bound: 2^-24 * 1e3 * rstd / max|y| ~ 1e-5)
    assert all(ok[n] for n in K.LN_GRAD_STRESS), ok
    assert "mean1e3" not in K.LN_GRAD_STRESS
    # the E[x^2] - E[x]^2 form is what the mean-1e3 row is there to expose: in f32 its variance is off by O(1)
    naive_var = float((x[1] * x[1]).mean() - x[1].mean() ** 2)
    true_var = float(((x[1].double() - x[1].double().mean()) ** 2).mean())
    assert abs(naive_var - true_var) > 1e-3 * true_var
    assert abs(float(1.0 / rstd32[1] ** 2 - 1e-5) - true_var) < 1e-5 * true_var


def test_sum_bound_covers_an_f32_running_sum():
    g = torch.Generator().manual_seed(0)
    t = torch.randn(70001, 64, generator=g)
    ref = t.double().sum(0)
    acc = torch.zeros(64)
    for c in t.split(997):                                            # a running f32 sum of f32 partial sums
        acc = acc + c.sum(0)
    bound = K.sum_bound(t.shape[0], t.double().abs().sum(0))
    assert bool(((acc.double() - ref).abs() <= bound).all())
