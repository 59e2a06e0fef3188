"""The split attention backward (``pgca_attention_bwd_split``: a dK/dV role per 128-key block, a dQ role per 128-query
block) past the 512 tokens of the one-pass kernel, and the first tests of the forward at those lengths: GPT-2's 1024
positions, ViT-L/14@336's 577 tokens.  Tolerances are the project's attention constants (tests/test_kernels_gpu.py,
tests/test_attention_tiled_gpu.py): out 1/64, lse 2e-3, dqkv 1/40 of the reference's maximum, cosine >= 0.9995 for
each of dq / dk / dv, masked keys exactly zero.  Where both backward entries run, they must agree bit for bit: the split
kernels keep the one-pass kernel's products and its order of summation."""
import pytest
import torch

from test_kernels_gpu import attn_ref, close, dev, drop_mult, hip, rnd  # noqa: F401  (hip is a fixture)

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


def _mask(S, lens):
    return (torch.arange(S)[None] < torch.tensor(lens)[:, None]).int().to(dev())


def _check_against_torch(hip, B, S, heads, causal, mask, seed):
    H = heads * 64
    qkv = rnd(B * S, 3 * H, seed=seed).bfloat16()
    out = torch.full((B * S, H), SENTINEL, dtype=torch.bfloat16, device=dev())
    lse = torch.zeros(B, heads, S, device=dev())
    hip.attention_fwd(qkv, mask, B, S, heads, causal, out, lse)
    x = qkv.float().requires_grad_()
    ref, ref_lse = attn_ref(x, mask, B, S, heads, causal)
    close(out, ref, 1.0 / 64, "attn out")
    lse_err = float((lse - ref_lse).abs().max())
    print(f"S={S} lse err {lse_err:.3e}")
    assert lse_err <= 2e-3
    valid = (mask.view(B * S, 1) != 0).float()
    dout = (rnd(B * S, H, seed=7) * valid).bfloat16()
    ref.backward(dout.float())
    dqkv = torch.full((B * S, 3 * H), SENTINEL, dtype=torch.bfloat16, device=dev())
    hip.attention_bwd_split(qkv, out, dout, lse, mask, B, S, heads, causal, dqkv)
    scale = float(x.grad.abs().max())
    print(f"S={S} dqkv err {float((dqkv.float() - x.grad).abs().max()) / scale:.3e} of the reference's maximum")
    close(dqkv, x.grad, 1.0 / 40, "attn dqkv")
    for name, sl in (("dq", slice(0, H)), ("dk", slice(H, 2 * H)), ("dv", slice(2 * H, 3 * H))):
        a, b = dqkv[:, sl].float().flatten().double(), x.grad[:, sl].flatten().double()
        cos = float(a @ b / (a.norm() * b.norm()))
        print(f"S={S} {name} cosine {cos:.6f}")
        assert cos >= 0.9995, name
    masked = (mask.view(-1) == 0)
    if bool(masked.any()):   # masked keys receive exactly zero gradient
        assert float(dqkv[masked][:, H:].abs().max()) == 0.0


# ragged right-padded lengths: a length of 1, and lengths that end one row into a 128-row block (513, 385, 257, 641, 897)
@pytest.mark.parametrize("cfg", [(2, 513, 1, True, [513, 1]), (2, 577, 2, False, [577, 385]),
                                 (2, 640, 2, True, [640, 257]), (3, 700, 1, False, [700, 1, 641]),
                                 (2, 1024, 2, True, [1024, 897]), (1, 1024, 1, False, [1024])],
                         ids=lambda c: f"B{c[0]}-S{c[1]}-h{c[2]}-{'causal' if c[3] else 'full'}")
def test_split_backward_against_torch(hip, cfg):
    B, S, heads, causal, lens = cfg
    _check_against_torch(hip, B, S, heads, causal, _mask(S, lens), seed=S + B)


@pytest.mark.parametrize("cfg", [(2, 129, 1, True, 0.0), (2, 300, 2, False, 0.0), (2, 512, 1, True, 0.0),
                                 (3, 256, 2, True, 0.1), (2, 300, 2, False, 0.1), (2, 385, 1, True, 0.1)],
                         ids=lambda c: f"B{c[0]}-S{c[1]}-h{c[2]}-{'causal' if c[3] else 'full'}-p{c[4]}")
def test_split_backward_is_the_one_pass_arithmetic(hip, cfg):
    """dK / dV sum over the query blocks in ascending order, dQ adds a fresh partial per key block in ascending order, as
    the one-pass kernel does: the same bits."""
    B, S, heads, causal, p = cfg
    H = heads * 64
    qkv = rnd(B * S, 3 * H, seed=S).bfloat16()
    mask = _mask(S, [S, max(1, S // 2 + 3), 1][:B])
    d = hip.drop_args(4321, p)
    out = torch.zeros(B * S, H, dtype=torch.bfloat16, device=dev())
    lse = torch.zeros(B, heads, S, device=dev())
    hip.attention_fwd(qkv, mask, B, S, heads, causal, out, lse, drop=d)
    dout = (rnd(B * S, H, seed=7) * (mask.view(B * S, 1) != 0).float()).bfloat16()
    one = torch.full((B * S, 3 * H), SENTINEL, dtype=torch.bfloat16, device=dev())
    two = torch.full((B * S, 3 * H), -SENTINEL, dtype=torch.bfloat16, device=dev())
    hip.attention_bwd(qkv, out, dout, lse, mask, B, S, heads, causal, one, drop=d)
    hip.attention_bwd_split(qkv, out, dout, lse, mask, B, S, heads, causal, two, drop=d)
    differ = int((one.view(torch.int16) != two.view(torch.int16)).sum())
    print(f"S={S}: {differ} of {one.numel()} elements differ")
    assert torch.equal(two, one)


def test_split_backward_mask_with_holes(hip):
    """Keys masked INSIDE a sequence (not only right padding), in three different key blocks."""
    B, S, heads = 2, 640, 1
    mask = torch.ones(B, S, dtype=torch.int32)
    mask[1, 5] = 0
    mask[1, 300:311] = 0
    mask[1, 600] = 0
    _check_against_torch(hip, B, S, heads, True, mask.to(dev()), seed=21)


def test_split_backward_dropout_replay(hip):
    """The backward replays the forward's counter-hash mask (the oracle's restatement of it), index
    ((b*heads + h)*S + q)*S + key, across key and query blocks."""
    B, S, heads = 3, 640, 2
    H = heads * 64
    qkv = rnd(B * S, 3 * H, seed=11).bfloat16()
    mask = _mask(S, [640, 530, 16])
    d = hip.drop_args(12345, 0.1)
    out = torch.zeros(B * S, H, dtype=torch.bfloat16, device=dev())
    lse = torch.zeros(B, heads, S, device=dev())
    hip.attention_fwd(qkv, mask, B, S, heads, True, out, lse, drop=d)
    mult = drop_mult(12345, 0.1, (B, heads, S, S))
    x = qkv.float().requires_grad_()
    q, k, v = x.view(B, S, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * 0.125
    allowed = torch.tril(torch.ones(S, S, dtype=torch.bool, device=dev()))[None, None] & (mask[:, None, None, :] != 0)
    p = torch.softmax(s.masked_fill(~allowed, float("-inf")), -1) * mult
    ref = (p @ v).permute(0, 2, 1, 3).reshape(B * S, H)
    close(out, ref, 1.0 / 64, "attn + prob dropout")
    valid = (mask.view(B * S, 1) != 0).float()
    dout = (rnd(B * S, H, seed=7) * valid).bfloat16()
    ref.backward(dout.float())
    dqkv = torch.full((B * S, 3 * H), SENTINEL, dtype=torch.bfloat16, device=dev())
    hip.attention_bwd_split(qkv, out, dout, lse, mask, B, S, heads, True, dqkv, drop=d)
    close(dqkv, x.grad, 1.0 / 40, "attn bwd with replayed dropout")


def test_split_backward_packed_rows_equal_padded(hip):
    """The ``cu`` launch on the packed rows equals the padded launch row for row (tests/test_packed_gpu.py's check on
    the new entry): masks, lse and dropout indices stay keyed on the padded (b, t) with row length Sp."""
    from pgca_amd.engine import make_row_pack
    S, heads, lens = 1024, 2, [1024, 513, 1, 130, 700, 512]
    B, H = len(lens), heads * 64
    g = torch.Generator().manual_seed(11)
    mask = _mask(S, lens)
    qkv = (torch.randn(B * S, 3 * H, generator=g)).bfloat16().to(dev())
    dout = (torch.randn(B * S, H, generator=g)).bfloat16().to(dev())
    dout = dout * mask.reshape(-1, 1).to(dout.dtype)   # a padded query has no gradient (its loss weight is zero)
    d = hip.drop_args(1234, 0.1)
    out, lse = torch.zeros(B * S, H, dtype=torch.bfloat16, device=dev()), torch.zeros(B, heads, S, device=dev())
    dqkv = torch.zeros(B * S, 3 * H, dtype=torch.bfloat16, device=dev())
    hip.attention_fwd(qkv, mask, B, S, heads, True, out, lse, drop=d)
    hip.attention_bwd_split(qkv, out, dout, lse, mask, B, S, heads, True, dqkv, drop=d)
    pk = make_row_pack(mask)
    rows = pk.row_ids[:pk.n].long()
    qkv_p = torch.zeros(pk.Mp, 3 * H, dtype=torch.bfloat16, device=dev())
    dout_p = torch.zeros(pk.Mp, H, dtype=torch.bfloat16, device=dev())
    qkv_p[:pk.n], dout_p[:pk.n] = qkv[rows], dout[rows]
    out_p = torch.full((pk.Mp, H), float("nan"), dtype=torch.bfloat16, device=dev())
    lse_p = torch.zeros(pk.nseq, heads, S, device=dev())
    dqkv_p = torch.full((pk.Mp, 3 * H), float("nan"), dtype=torch.bfloat16, device=dev())
    hip.attention_fwd(qkv_p, pk.mask, pk.nseq, S, heads, True, out_p, lse_p, drop=d, cu=pk.cu)
    hip.attention_bwd_split(qkv_p, out_p, dout_p, lse_p, pk.mask, pk.nseq, S, heads, True, dqkv_p, drop=d, cu=pk.cu)
    assert torch.equal(out_p[:pk.n], out[rows]), "forward rows differ"
    for b, n in enumerate(lens):
        assert torch.equal(lse_p[b, :, :n], lse[b, :, :n])
    assert torch.equal(dqkv_p[:pk.n], dqkv[rows]), "backward rows differ"
    # the filler rows are an ordinary (finite) sequence of zero inputs: zero gradient, finite output
    assert bool(torch.isfinite(out_p.float()).all())
    assert float(dqkv_p[pk.n:].float().abs().max() if pk.Mp > pk.n else 0) == 0.0


def test_split_backward_is_reproducible(hip):
    """No atomics, nothing summed across workgroups: two launches on the same inputs are bitwise equal."""
    B, S, heads = 4, 768, 4
    H = heads * 64
    qkv = rnd(B * S, 3 * H, seed=5).bfloat16()
    mask = _mask(S, [768, 387, 767, 1])
    dout = rnd(B * S, H, seed=9).bfloat16()
    res = []
    for _ in range(2):
        out = torch.zeros(B * S, H, dtype=torch.bfloat16, device=dev())
        lse = torch.zeros(B, heads, S, device=dev())
        dqkv = torch.zeros(B * S, 3 * H, dtype=torch.bfloat16, device=dev())
        hip.attention_fwd(qkv, mask, B, S, heads, True, out, lse)
        hip.attention_bwd_split(qkv, out, dout, lse, mask, B, S, heads, True, dqkv)
        res.append((out.clone(), lse.clone(), dqkv.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
