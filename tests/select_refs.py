"""Plain float64 restatements of the rules of the two selection kernels (``csrc/select.hip``): HF's processors as
``CaptionDecoder._process_scores`` applies them (plus top-k), the inverse-CDF draw in token-id order, the beam
candidates' ranking and its Gumbel keys with a Python ``hash32``.  Shared by ``test_select_refs_cpu.py`` (which ties
them to ``oracle.restatement.process_scores`` and to ``row_kernel_refs.drop_mult_at``) and ``test_select_gpu.py``.

Nothing here knows about waves or passes: whole-tensor formulas, with a sort where the kernels use a radix select.
"""
import torch

F64 = torch.float64
_M32 = 0xFFFFFFFF
NEG_INF = float("-inf")


def hash32(x: torch.Tensor) -> torch.Tensor:
    """``hash32`` of csrc/common.h (lowbias32) on int64 tensors holding uint32 values."""
    x = x & _M32
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & _M32
    x = x ^ (x >> 16)
    return x


def gumbel(flat: torch.Tensor, seed: int) -> torch.Tensor:
    """g = -log(-log u), u = ((hash32(flat * 0x9E3779B1 + seed) >> 8) + 0.5) * 2^-24, float64."""
    h = hash32(((flat & _M32) * 0x9E3779B1 + (seed & _M32)) & _M32)
    u = ((h >> 8).to(F64) + 0.5) * 2.0 ** -24
    return -torch.log(-torch.log(u))


def top_k_filter(s: torch.Tensor, top_k: int) -> torch.Tensor:
    """Scores strictly below the k-th largest go; ties with it stay; 0 or >= V is off."""
    if not 0 < top_k < s.shape[-1]:
        return s
    kth = torch.sort(s, dim=-1, descending=True)[0][:, top_k - 1:top_k]
    return s.masked_fill(s < kth, NEG_INF)


def top_p_removed(s: torch.Tensor, top_p: float):
    """HF's rule with classes of equal score kept or removed together: ascending, a class goes iff the cumulative
    probability up to and including its LAST member is <= 1 - top_p; the largest stays.  Returns (removed mask [R, V],
    cumulative masses [R, V] in ascending order: what the redraw condition of the tests looks at)."""
    srt, idx = torch.sort(s, dim=-1, descending=False, stable=True)
    cum = torch.softmax(srt, dim=-1).cumsum(dim=-1)
    last = torch.searchsorted(srt.contiguous(), srt.contiguous(), right=True) - 1
    rm = torch.gather(cum, 1, last) <= (1.0 - float(top_p))
    rm[:, -1] = False
    rm = rm & (srt >= srt[:, -1:]).logical_not()
    return torch.zeros_like(rm).scatter(1, idx, rm), cum


def process(scores: torch.Tensor, prev: torch.Tensor, repetition_penalty: float, warp: bool, temperature: float = 1.0,
            top_k: int = 0, top_p: float = 1.0) -> torch.Tensor:
    """float64 processed scores, removed tokens -inf.  The penalty acts once per distinct id of ``prev``."""
    s = scores.to(F64)
    if repetition_penalty != 1.0 and prev.shape[1]:
        seen = torch.zeros_like(s, dtype=torch.bool).scatter(1, prev, True)
        s = torch.where(seen, torch.where(s < 0, s * repetition_penalty, s / repetition_penalty), s)
    if warp:
        s = s / float(temperature)
        s = top_k_filter(s, top_k)
        if top_p < 1.0:
            s = s.masked_fill(top_p_removed(s, top_p)[0], NEG_INF)
    return s


def first_max(s: torch.Tensor) -> torch.Tensor:
    return (s == s.max(dim=-1, keepdim=True)[0]).to(torch.int8).argmax(dim=-1)


def select_token(logits, prev, repetition_penalty, temperature, top_k, top_p, u, done, pad_id):
    """(next [R] int64, next_logp [R] float64, margin [R]): ``margin`` is the distance of the row from an undecidable
    input - a cumulative mass next to 1 - top_p, or u * Z next to a CDF step - in units of probability."""
    x = logits.to(F64)
    lp = torch.log_softmax(x, dim=-1)
    R = x.shape[0]
    margin = torch.full((R,), float("inf"), dtype=F64)
    if u is None:
        nxt = first_max(process(x, prev, repetition_penalty, False))
    else:
        s = process(x, prev, repetition_penalty, True, temperature, top_k, top_p)
        if top_p < 1.0:
            pre = top_k_filter(process(x, prev, repetition_penalty, True, temperature), top_k)
            cum = top_p_removed(pre, top_p)[1]
            if cum.shape[1] > 1:    # the largest always stays: its own cumulative mass (1) decides nothing
                margin = (cum[:, :-1] - (1.0 - float(top_p))).abs().min(dim=-1)[0]
        p = torch.exp(s - s.max(dim=-1, keepdim=True)[0])
        cdf = p.cumsum(dim=-1)
        z = cdf[:, -1:]
        target = u.to(F64)[:, None] * z
        nxt = (cdf >= target).to(torch.int8).argmax(dim=-1)
        margin = torch.minimum(margin, ((cdf - target) / z).abs().min(dim=-1)[0])
    nlp = lp.gather(1, nxt[:, None])[:, 0]
    if done is not None:
        nxt = torch.where(done.bool(), torch.full_like(nxt, pad_id), nxt)
        nlp = torch.where(done.bool(), torch.zeros_like(nlp), nlp)
    return nxt, nlp, margin


def beam_candidates(logits, B, nb, prev, repetition_penalty, warp, temperature, top_k, top_p, beam_scores, K, use_noise,
                    noise_seed):
    """(cand_score [B, K] float64, cand_index [B, K] int64, keys [B, K + 1] sorted descending): the processors on the
    log-probabilities, acc = processed + beam score, key = acc (+ Gumbel noise of the GLOBAL flat index), ranked by key
    descending and flat index ascending (a stable sort), -inf keys last."""
    V = logits.shape[1]
    lp = torch.log_softmax(logits.to(F64), dim=-1)
    s = process(lp, prev, repetition_penalty, warp, temperature, top_k, top_p)
    acc = (s + beam_scores.to(F64).reshape(-1, 1)).view(B, nb * V)
    key = acc
    if use_noise:
        flat = torch.arange(B * nb * V, dtype=torch.int64).view(B, nb * V)
        key = torch.where(torch.isinf(acc), acc, acc + gumbel(flat, noise_seed))
    srt, order = torch.sort(-key, dim=-1, stable=True)
    return torch.gather(acc, 1, order[:, :K]), order[:, :K], -srt[:, :K + 1]
