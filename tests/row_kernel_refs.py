"""Plain float64 references of the row kernels (attention, LayerNorm, the caption-decoder embedding) with HAND-WRITTEN
backward formulas, shared by ``test_bench_geometry_rows_gpu.py`` (which runs them on the device, in chunks, next to the
kernels) and ``test_row_kernel_references_cpu.py`` (which checks every formula here against ``torch.autograd``).

Nothing here knows about tiles, waves or launch geometry: every function is the textbook formula on whole tensors, on
whatever device its inputs live.
"""
import torch

F64 = torch.float64
_M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ dropout hash
def drop_mult_at(seed: int, p: float, idx: torch.Tensor) -> torch.Tensor:
    """``oracle.restatement.dropout_multiplier`` evaluated at arbitrary element indices (int64, any shape, taken modulo
    2^32 as the kernels' unsigned index arithmetic does): float64 0 / 1/(1-p), with 1/(1-p) the FLOAT32 value the
    kernels multiply by."""
    idx = idx & _M32
    x = ((idx >> 1) * 0x9E3779B1 + (seed & _M32)) & _M32
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & _M32
    x = x ^ (x >> 16)
    bits = torch.where((idx & 1) == 1, x >> 16, x & 0xFFFF)
    keep = bits >= (min(_M32, int(p * 4294967296.0)) >> 16)
    scale = float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float32))
    return keep.to(F64) * scale


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    """float64 -> nearest bfloat16 (through float32, as the kernels' accumulators are) -> float64."""
    return x.float().bfloat16().to(F64)


# ------------------------------------------------------------------------------------------------ attention
def attn_allowed(key_mask: torch.Tensor, S: int, causal: bool) -> torch.Tensor:
    """[b, 1, S, S] bool: key allowed for query = (key <= query if causal) AND key_mask[b, key] != 0."""
    al = torch.ones(S, S, dtype=torch.bool, device=key_mask.device)
    if causal:
        al = torch.tril(al)
    return al[None, None] & (key_mask[:, None, None, :] != 0)


def attn_drop_mult(seed: int, p: float, b0: int, nb: int, heads: int, S: int, device) -> torch.Tensor:
    """Probability-dropout multipliers of sequences b0 .. b0+nb-1: element index ((b*heads + h)*S + q)*S + key."""
    n = nb * heads * S * S
    idx = torch.arange(n, dtype=torch.int64, device=device) + b0 * heads * S * S
    return drop_mult_at(seed, p, idx).view(nb, heads, S, S)


def _softmax_parts(q, k, allowed):
    s = (q @ k.transpose(-1, -2)) * 0.125
    s = s.masked_fill(~allowed, float("-inf"))
    m = s.amax(-1, keepdim=True)
    m0 = torch.where(torch.isinf(m), torch.zeros_like(m), m)       # a query with no allowed key: all e = 0
    e = torch.exp(s - m0)
    l = e.sum(-1, keepdim=True)
    lse = (m0 + torch.log(l)).squeeze(-1)                           # log(0) = -inf for such a query
    return s, e, l, lse


def attn_fwd_ref(q, k, v, allowed, mult=None):
    """q, k, v float64 [b, h, S, 64].  Returns out [b, h, S, 64], lse [b, h, S], P (undropped) [b, h, S, S].
    A query with no allowed key has P = 0, out = 0, lse = -inf (the kernels' contract, include/pgca_hip.h)."""
    _, e, l, lse = _softmax_parts(q, k, allowed)
    P = e / torch.where(l > 0, l, torch.ones_like(l))
    Pd = P if mult is None else P * mult
    return Pd @ v, lse, P


def attn_bwd_ref(q, k, v, dout, allowed, mult=None):
    """Hand-written backward of ``attn_fwd_ref``: dq, dk, dv."""
    out, _, P = attn_fwd_ref(q, k, v, allowed, mult)
    Pd = P if mult is None else P * mult
    dv = Pd.transpose(-1, -2) @ dout
    dPd = dout @ v.transpose(-1, -2)
    dP = dPd if mult is None else dPd * mult
    delta = (dout * out).sum(-1, keepdim=True)                       # = sum_key P dP
    dS = P * (dP - delta) * 0.125
    return dS @ k, dS.transpose(-1, -2) @ q, dv


def attn_emulated(q, k, v, dout, allowed, mult=None):
    """The same formulas in float64 with the kernels' documented ROUNDING POINTS inserted (attention_tiled.hip): the
    dropped, un-normalised probability exp(s - max) * m is rounded to bf16 before P V, the output is rounded to bf16; the
    backward recomputes p = exp(s - lse), takes delta from the ROUNDED output, rounds p * m and dS to bf16 before the
    three products and rounds dq / dk / dv to bf16.  Its distance from the pure float64 result is the error a correct
    kernel is entitled to; summation order and the hardware exp / log are not modelled (the factor on top of it)."""
    s, e, l, lse = _softmax_parts(q, k, allowed)
    em = e if mult is None else e * mult
    out = bf16_round((bf16_round(em) @ v) / torch.where(l > 0, l, torch.ones_like(l)))
    lse_f = torch.where(torch.isinf(lse), torch.zeros_like(lse), lse)[..., None]
    pu = torch.where(allowed, torch.exp(s.masked_fill(~allowed, 0.0) - lse_f), torch.zeros_like(s))
    one = torch.ones((), dtype=F64, device=q.device) if mult is None else mult
    delta = (dout * out).sum(-1, keepdim=True)
    dPd = dout @ v.transpose(-1, -2)
    ds = bf16_round(pu * (dPd * one - delta) * 0.125)
    pd = bf16_round(pu * one)
    dq, dk, dv = ds @ k, ds.transpose(-1, -2) @ q, pd.transpose(-1, -2) @ dout
    return out, bf16_round(dq), bf16_round(dk), bf16_round(dv)


def split_heads(x, nb, S, heads):
    """[nb*S, heads*64] -> [nb, heads, S, 64] float64."""
    return x.to(F64).view(nb, S, heads, 64).permute(0, 2, 1, 3)


def merge_heads(x):
    """[nb, heads, S, 64] -> [nb*S, heads*64]."""
    nb, heads, S, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(nb * S, heads * 64)


def sharp_qkv(nb, S, heads, gen, shift_head=0):
    """The SHARP input distribution, as float32 [nb*S, 3*heads*64] (to be rounded to bf16 by the caller):

    * q, k ~ 2.83 N(0, 1) in 63 of the 64 head dimensions: scores q.k / 8 have standard deviation 8 * sqrt(63/64);
    * dimension 63 is the SINK channel: q[., 63] = 8 for every query, k[0, 63] = 60 for key 0 and 0 elsewhere, so key 0's
      score is raised by 8 * 60 / 8 = +60 for every query (all values exact in bf16);
    * head ``shift_head``: k[., 63] = -80 for EVERY key, key 0 included: all its scores are shifted by 8 * -80 / 8 = -80.
      The sink is left out of this one head: at -80 + 60 it would put every row maximum back at -20, where float32
      survives a missing maximum subtraction; without it the rows sit at e^-80 .. e^-110, below the float32 normal range
      (e^-87.3) for about every sixth single-key row, so only a kernel that subtracts the maximum gets them right.
    """
    H = heads * 64
    x = torch.randn(nb * S, 3, heads, 64, generator=gen, device=gen.device)
    x[:, 0:2] *= 8.0 ** 0.5
    x[:, 0, :, 63] = 8.0
    x[:, 1, :, 63] = 0.0
    xs = x.view(nb, S, 3, heads, 64)
    xs[:, 0, 1, :, 63] = 60.0
    xs[:, :, 1, shift_head, 63] = -80.0
    return x.view(nb * S, 3 * H)


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_fwd_ref(x, gamma, beta, eps=1e-5):
    """float64 two-pass LayerNorm of rows x [M, H]: y, mean [M], rstd [M]."""
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x - mean) * rstd * gamma + beta, mean.squeeze(-1), rstd.squeeze(-1)


def ln_bwd_ref(x, gamma, dy, eps=1e-5):
    """Hand-written LayerNorm backward: dx [M, H] plus the TERMS of the column sums (dgamma = sum_m dy * xhat,
    dbeta = sum_m dy), returned per row so that a caller can also form sum |terms|."""
    H = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    xh = (x - mean) * rstd
    g = dy * gamma
    c1 = g.sum(-1, keepdim=True) / H
    c2 = (g * xh).sum(-1, keepdim=True) / H
    return rstd * (g - c1 - xh * c2), dy * xh, dy


def ln_bwd_full_ref(x, gamma, dy, add_to, m_add, m_dx, eps=1e-5):
    """``pgca_layernorm_bwd`` with everything on: dx_out = add_to + dx (never masked), dx_bf16 = dx_out * m_dx (before its
    rounding), and the four column-sum term planes dgamma, dbeta, add_to * m_add, dx_out * m_dx."""
    dx, tg, tb = ln_bwd_ref(x, gamma, dy, eps)
    dx_out = dx + add_to
    return dx_out, dx_out * m_dx, (tg, tb, add_to * m_add, dx_out * m_dx)


# ------------------------------------------------------------------------------------------------ embedding
def embed_fwd_ref(ids, wte, wpe, att, U, w, gamma, beta, me, eps=1e-5):
    """Caption-decoder input of positions (b, s), all float64: ids [B, S]; att [B, H] or [H] (b_o alone); U [B, XH, H] with
    head weights w [B, XH, S] (or None); me [B, S, H] embedding-dropout multipliers (or None).
    h0 = (LN(wte[id] + att + sum_h w U) + wpe[s]) * me.  Returns h0 [B, S, H] and e (the LN input)."""
    B, S = ids.shape
    e = wte[ids] + (att[None, None, :] if att.dim() == 1 else att[:, None, :])
    if U is not None:
        e = e + torch.einsum("bhs,bhc->bsc", w, U)
    y, _, _ = ln_fwd_ref(e.reshape(B * S, -1), gamma, beta, eps)
    h0 = y.view(B, S, -1) + wpe[:S][None]
    return (h0 if me is None else h0 * me), e


EMBED_PER_SEQUENCE = ("datt", "abs_datt", "rs_datt", "dU", "abs_dU", "rs_dU")   # results with one row per sequence


def embed_bwd_ref(g, ids, rmask, e, U, w, gamma, me, V, eps=1e-5):
    """Hand-written backward of ``embed_fwd_ref`` for g = dL/dh0 [B, S, H]; positions with rmask [B, S] == 0 contribute
    nothing.  Returns dict(dwte [V, H], dwpe [S, H], datt [B, H], dU [B, XH, H] or None, dgamma, dbeta and the |term|
    sums ``abs_*`` that bound the accumulation error of each)."""
    B, S, H = g.shape
    r = (rmask != 0).to(F64)[..., None]
    gd = (g if me is None else g * me) * r
    de, tg, tb = ln_bwd_ref(e.reshape(B * S, H), gamma, gd.reshape(B * S, H), eps)
    de = de.view(B, S, H) * r
    flat = ids.reshape(-1)
    rs = de.abs().amax(-1)                                            # [B, S]: the row scale of every term de[b, s, :]
    zV = lambda *sh: torch.zeros(*sh, dtype=F64, device=g.device)     # noqa: E731
    res = {"dwte": zV(V, H).index_add_(0, flat, de.reshape(B * S, H)),
           "abs_dwte": zV(V, H).index_add_(0, flat, de.abs().reshape(B * S, H)),
           "n_dwte": zV(V).index_add_(0, flat, r.reshape(-1)), "rs_dwte": zV(V).index_add_(0, flat, rs.reshape(-1)),
           "dwpe": gd.sum(0), "abs_dwpe": gd.abs().sum(0),
           "datt": de.sum(1), "abs_datt": de.abs().sum(1), "rs_datt": rs.sum(1),
           "dgamma": tg.sum(0), "abs_dgamma": tg.abs().sum(0), "dbeta": tb.sum(0), "abs_dbeta": tb.abs().sum(0),
           "dU": None}
    if U is not None:
        res["dU"] = torch.einsum("bhs,bsc->bhc", w, de)
        res["abs_dU"] = torch.einsum("bhs,bsc->bhc", w, de.abs())
        res["rs_dU"] = torch.einsum("bhs,bs->bh", w, rs)
    return res


# ------------------------------------------------------------------------------------------------ error measures
def row_errors(got, ref, floor_frac):
    """Per-row relative error: max_c |got[r, c] - ref[r, c]| / (max_c |ref[r, c]| + floor_frac * max |ref|).
    Returns (errors [rows], scale [rows])."""
    got, ref = got.to(F64), ref.to(F64)
    scale = ref.abs().amax(-1) + floor_frac * ref.abs().max()
    return (got - ref).abs().amax(-1) / scale, scale


def cosine(a, b):
    a, b = a.to(F64).flatten(), b.to(F64).flatten()
    return float(a @ b / (a.norm() * b.norm()))


def sum_bound(n_terms, abs_sum):
    """Bound of an f32 sum of ``n_terms`` terms in an arbitrary order: sqrt(n) * eps_f32 * sum |terms| (the random-walk
    growth of the rounding error of a running sum whose partial sums are bounded by sum |terms|), plus one f32 rounding
    of the result."""
    eps = 2.0 ** -24
    n = n_terms if torch.is_tensor(n_terms) else torch.tensor(float(n_terms), dtype=F64, device=abs_sum.device)
    return (torch.sqrt(n.clamp(min=1.0)) + 1.0) * eps * abs_sum


LN_STRESS = ("constant", "mean1e3", "outlier1e4")
# the stress rows that a correctly rounded f32 two-pass LayerNorm carries within the gradient bounds (derived from float64 in
# test_row_kernel_references_cpu.py::test_layernorm_stress_rows_against_a_rounded_f32_two_pass, not from a kernel)
LN_GRAD_STRESS = ("constant", "outlier1e4")


def ln_stress_rows(H, gen):
    """Three float32 rows that stress the variance: a constant row (variance 0 -> rstd = 1/sqrt(eps)), mean 1e3 with unit
    spread (E[x^2] - E[x]^2 cancels catastrophically in f32), one 1e4 outlier among unit normals."""
    a = torch.full((H,), 3.25, device=gen.device)
    b = 1000.0 + torch.randn(H, generator=gen, device=gen.device)
    c = torch.randn(H, generator=gen, device=gen.device)
    c[H // 3] = 1e4
    return torch.stack([a, b, c])


def ln_stress_fwd_bound(x_row, gamma, y_row, rstd):
    """Absolute bound on y of a stress row: the per-row 1e-5 of the row scale, plus the float32 rounding of the mean and of
    x - mean (2 * 2^-24 * max |x| each) carried through rstd * |gamma|."""
    return 1e-5 * y_row.abs().max() + 4 * 2.0 ** -24 * x_row.abs().max() * rstd * gamma.abs().max()


def f32_two_pass_ln(x32, gamma32, beta32, eps=1e-5):
    """A correctly rounded float32 two-pass LayerNorm (every operation in f32, sums by torch): what the kernels compute up
    to summation order."""
    mean = x32.mean(-1, keepdim=True)
    var = ((x32 - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32, device=x32.device))
    return (x32 - mean) * rstd * gamma32 + beta32, mean.squeeze(-1), rstd.squeeze(-1)

