"""The attention forward in its K/V-cache form (what ``GptTrunk.decode_step`` launches every step): ``cu[r] = r * smax``
is the cache STRIDE and ``S`` the filled length, no key mask, no lse.  The cache comes from ``torch.empty``, so whatever
lies in rows >= S - NaN bit patterns included - must neither be read into a result nor be written over.  Every row
>= S of the cache is therefore poisoned with NaN here and the output prefilled with a sentinel; the reference is plain
float64 softmax attention on the CPU over rows 0 .. S-1 only, so it never sees the poison.

Measured on the MI355X over the 20 cases: worst error 9.4e-3 on outputs of magnitude 2.4 - 3.9, at most 3.7e-3 of the
scale (S = 127 of 130, three sequences) against the bound of 1/64 = 1.6e-2; S = 1 is exact."""
import pytest
import torch

from test_kernels_gpu import close, dev, hip, rnd  # noqa: F401  (hip is a fixture)

pytestmark = pytest.mark.gpu

HEADS, DH = 2, 64
SENTINEL = 7.0
# one-tile kernel (S <= 128) / the 128|129 switch to the eight-wave online-softmax kernel / 16-row edges inside a tile /
# a third key tile / S == smax against S < smax
SHAPES = [(16, 1), (16, 16), (130, 17), (130, 127), (130, 128), (130, 129), (130, 130), (300, 256), (300, 257), (300, 300)]


def _reference(qkv, S):
    """Causal softmax attention of the first ``S`` rows of one sequence, float64: [S, heads * 64]."""
    q, k, v = qkv[:S].double().view(S, 3, HEADS, DH).permute(1, 2, 0, 3)        # each [heads, S, 64]
    s = (q @ k.transpose(-1, -2)) * DH ** -0.5
    s = s.masked_fill(~torch.tril(torch.ones(S, S, dtype=torch.bool)), float("-inf"))
    return (torch.softmax(s, dim=-1) @ v).permute(1, 0, 2).reshape(S, HEADS * DH)


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("smax,S", SHAPES)
def test_cache_form_attention_reads_and_writes_only_the_filled_rows(hip, R, smax, S):
    H = HEADS * DH
    qkv = rnd(R * smax, 3 * H, seed=1000 * smax + 10 * S + R).bfloat16()
    qkv.view(R, smax, 3 * H)[:, S:] = float("nan")
    cu = (torch.arange(R + 1, dtype=torch.int32) * smax).to(dev())
    out = torch.full((R * smax, H), SENTINEL, dtype=torch.bfloat16, device=dev())
    hip.attention_fwd(qkv, None, R, S, HEADS, True, out, None, cu=cu)
    got = out.cpu().view(R, smax, H)
    host = qkv.cpu().view(R, smax, 3 * H)
    want = torch.stack([_reference(host[r], S) for r in range(R)])
    assert bool(torch.isfinite(want).all())
    filled = got[:, :S].float()
    finite = bool(torch.isfinite(filled).all())
    err = float((filled.double() - want).abs().nan_to_num(nan=float("inf")).max())
    print(f"cache attention R={R} smax={smax} S={S}: max err {err:.3e} of scale {float(want.abs().max()):.3e}, "
          f"finite={finite}")
    assert finite, "a row < S picked up the poison of the rows >= S"
    close(filled, want, 1.0 / 64, "cache-form attention")
    assert torch.equal(got[:, S:], torch.full_like(got[:, S:], SENTINEL)), "a row >= S of the output was written"
