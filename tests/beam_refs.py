"""Torch restatements of what the ``_ex`` selection kernels and ``pgca_beam_step`` add (csrc/select.hip, csrc/beam.hip):
HF's banning processors (NoRepeatNGram, MinLength / MinNewTokensLength, SuppressTokens), one step of HF's beam-search
bookkeeping, and the beam loop built from the two.  ``test_beam_refs_cpu.py`` pins them against transformers' own
processors and ``generate``; the GPU tests compare the kernels and ``CaptionDecoder.generate`` with them.

Rankings use a STABLE sort: score descending, then index ascending (``torch.topk`` promises nothing for equal keys).
Nothing here knows about workgroups or ping-pong buffers.
"""
import torch

import select_refs as S

F64 = torch.float64
NEG_INF = float("-inf")


# ------------------------------------------------------------------------------------------------ banning processors
def ngram_banned_ids(prev_row, n):
    """HF NoRepeatNGramLogitsProcessor for one row (a list of ids): the ids that followed an earlier occurrence of the
    row's last n - 1 ids."""
    m = len(prev_row)
    if n <= 0 or m < n - 1:
        return []
    tail = list(prev_row[m - n + 1:]) if n > 1 else []
    return [prev_row[i + n - 1] for i in range(m - n + 1) if list(prev_row[i:i + n - 1]) == tail]


def ban_mask(prev, V, no_repeat_ngram_size=0, ban_ids=()):
    """bool [R, V]: True where the processed score is -inf.  Ids outside [0, V) are ignored."""
    R = prev.shape[0]
    mask = torch.zeros(R, V, dtype=torch.bool)
    for r in range(R):
        for t in ngram_banned_ids(prev[r].tolist(), int(no_repeat_ngram_size)) + [int(t) for t in ban_ids]:
            if 0 <= t < V:
                mask[r, t] = True
    return mask


def min_length_ban_ids(step, eos, min_new, suppress=()):
    """The list the Python side hands the kernels at ``step`` (tokens generated so far): ``suppress`` always, [EOS]
    while fewer than ``min_new`` tokens exist."""
    return list(suppress) + ([eos] if step < min_new else [])


def process(scores, prev, repetition_penalty, warp, temperature=1.0, top_k=0, top_p=1.0, no_repeat_ngram_size=0,
            ban_ids=()):
    """float64 processed scores in HF's order: repetition penalty, bans (-inf whatever came before), then the warpers."""
    s = S.process(scores, prev, repetition_penalty, False)
    s = s.masked_fill(ban_mask(prev, s.shape[1], no_repeat_ngram_size, ban_ids), NEG_INF)
    if warp:
        s = s / float(temperature)
        s = S.top_k_filter(s, top_k)
        if top_p < 1.0:
            s = s.masked_fill(S.top_p_removed(s, top_p)[0], NEG_INF)
    return s


def select_token(logits, prev, repetition_penalty, temperature, top_k, top_p, u, done, pad_id, no_repeat_ngram_size=0,
                 ban_ids=()):
    """``select_refs.select_token`` with the bans: (next, next_logp of the RAW row, margin).  A row with every token
    banned yields id 0."""
    x = logits.to(F64)
    lp = torch.log_softmax(x, dim=-1)
    R = x.shape[0]
    margin = torch.full((R,), float("inf"), dtype=F64)
    if u is None:
        nxt = S.first_max(process(x, prev, repetition_penalty, False, no_repeat_ngram_size=no_repeat_ngram_size,
                                  ban_ids=ban_ids))
    else:
        s = process(x, prev, repetition_penalty, True, temperature, top_k, top_p, no_repeat_ngram_size, ban_ids)
        dead = torch.isinf(s).all(dim=-1)
        s = torch.where(dead[:, None], torch.zeros_like(s), s)
        if top_p < 1.0:
            pre = S.top_k_filter(process(x, prev, repetition_penalty, True, temperature, 0, 1.0, no_repeat_ngram_size,
                                         ban_ids), top_k)
            pre = torch.where(dead[:, None], torch.zeros_like(pre), pre)
            cum = S.top_p_removed(pre, top_p)[1]
            if cum.shape[1] > 1:
                margin = torch.where(dead, margin, (cum[:, :-1] - (1.0 - float(top_p))).abs().min(dim=-1)[0])
        p = torch.exp(s - s.max(dim=-1, keepdim=True)[0])
        cdf = p.cumsum(dim=-1)
        z = cdf[:, -1:]
        target = u.to(F64)[:, None] * z
        nxt = (cdf >= target).to(torch.int8).argmax(dim=-1)
        margin = torch.where(dead, margin, torch.minimum(margin, ((cdf - target) / z).abs().min(dim=-1)[0]))
        nxt = torch.where(dead, torch.zeros_like(nxt), nxt)
    nlp = lp.gather(1, nxt[:, None])[:, 0]
    if done is not None:
        nxt = torch.where(done.bool(), torch.full_like(nxt, pad_id), nxt)
        nlp = torch.where(done.bool(), torch.zeros_like(nlp), nlp)
    return nxt, nlp, margin


def beam_candidates(logits, B, nb, prev, repetition_penalty, warp, temperature, top_k, top_p, beam_scores, K, use_noise,
                    noise_seed, no_repeat_ngram_size=0, ban_ids=()):
    """``select_refs.beam_candidates`` with the bans (the log-softmax is that of the RAW row)."""
    V = logits.shape[1]
    lp = torch.log_softmax(logits.to(F64), dim=-1)
    s = process(lp, prev, repetition_penalty, warp, temperature, top_k, top_p, no_repeat_ngram_size, ban_ids)
    acc = (s + beam_scores.to(F64).reshape(-1, 1)).view(B, nb * V)
    key = acc
    if use_noise:
        flat = torch.arange(B * nb * V, dtype=torch.int64).view(B, nb * V)
        key = torch.where(torch.isinf(acc), acc, acc + S.gumbel(flat, noise_seed))
    srt, order = torch.sort(-key, dim=-1, stable=True)
    return torch.gather(acc, 1, order[:, :K]), order[:, :K], -srt[:, :K + 1]


# ------------------------------------------------------------------------------------------------ one beam step
def top_stable(x, k):
    """Indices of the k largest entries of each row: value descending, index ascending among equals."""
    return torch.sort(-x, dim=-1, stable=True)[1][:, :k]


def new_state(B, nb, L, pad):
    """The state HF's ``_beam_search`` starts from (its names)."""
    rbs = torch.zeros(B, nb)
    rbs[:, 1:] = -1e9
    return dict(running_sequences=torch.full((B, nb, L), pad, dtype=torch.int64),
                sequences=torch.full((B, nb, L), pad, dtype=torch.int64), running_beam_scores=rbs,
                beam_scores=torch.full((B, nb), -1e9), is_sent_finished=torch.zeros(B, nb, dtype=torch.bool),
                gen_len=torch.zeros(B, nb, dtype=torch.int64), unsat=torch.ones(B, 1, dtype=torch.bool))


def beam_step(st, cand_score, cand_index, V, cur, L, eos, length_penalty=1.0, early_stopping=False):
    """Steps e, f, g of HF's ``_beam_search`` on float32 CPU tensors.  ``st``: a ``new_state`` dict (not modified).
    Returns (new state, tok [B * nb], flat_src [B * nb], hits_all [B])."""
    B, nb = st["beam_scores"].shape
    K = 2 * nb
    ar = torch.arange(B)[:, None]
    cand_score = cand_score.float()
    src_beam = cand_index // V
    topk_ids = cand_index % V
    topk_running = st["running_sequences"][ar, src_beam].clone()
    topk_running[:, :, cur] = topk_ids
    hits = (topk_ids == eos) | (cur + 1 >= L)
    # e. _get_running_beams_for_next_iteration
    run_lp = cand_score + hits.float() * -1.0e9
    nxt_idx = top_stable(run_lp, nb)
    out = dict(running_sequences=topk_running[ar, nxt_idx], running_beam_scores=torch.gather(run_lp, 1, nxt_idx))
    beam_src = torch.gather(src_beam, 1, nxt_idx)
    # f. _update_finished_beams
    just = hits & (torch.arange(K) < nb)[None, :]
    fin_lp = cand_score / ((cur + 1) ** length_penalty)
    full = st["is_sent_finished"].all(dim=-1, keepdim=True) & (early_stopping is True)
    fin_lp = fin_lp + full.float() * -1.0e9
    fin_lp = fin_lp + (~st["unsat"]).float() * -1.0e9
    fin_lp = fin_lp + (~just).float() * -1.0e9
    m_seq = torch.cat([st["sequences"], topk_running], dim=1)
    m_sc = torch.cat([st["beam_scores"], fin_lp], dim=1)
    m_fin = torch.cat([st["is_sent_finished"], just], dim=1)
    m_len = torch.cat([st["gen_len"], torch.full((B, K), cur + 1, dtype=torch.int64)], dim=1)
    keep = top_stable(m_sc, nb)
    out.update(sequences=m_seq[ar, keep], beam_scores=torch.gather(m_sc, 1, keep),
               is_sent_finished=torch.gather(m_fin, 1, keep), gen_len=torch.gather(m_len, 1, keep))
    # g. _check_early_stop_heuristic at cur_len = cur + 1
    hyp = L if (early_stopping == "never" and length_penalty > 0.0) else cur + 1
    best_run = out["running_beam_scores"][:, :1] / (hyp ** length_penalty)
    worst_fin = torch.where(out["is_sent_finished"], out["beam_scores"].min(dim=1, keepdim=True)[0],
                            torch.full_like(out["beam_scores"], -1.0e9))
    out["unsat"] = st["unsat"] & (best_run > worst_fin).any(dim=-1, keepdim=True)
    tok = torch.gather(topk_ids, 1, nxt_idx).reshape(-1)
    flat_src = (beam_src + ar * nb).reshape(-1)
    return out, tok, flat_src, hits.all(dim=-1)


def beam_search(logits_fn, B, nb, L, pad, eos, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new=0, suppress=(),
                length_penalty=1.0, early_stopping=False, eos_check=1):
    """Deterministic beam search as HF runs it, from the restatements above.  ``logits_fn(prev [B * nb, cur])`` returns
    the next-token logits [B * nb, V]; ``min_new`` counts generated tokens.  The stop flag is read every ``eos_check``
    steps (HF: 1).  Returns (sequences [B, nb, L] best first, beam_scores [B, nb], gen_len [B, nb])."""
    st = new_state(B, nb, L, pad)
    cur = 0
    while True:
        prev = st["running_sequences"].view(B * nb, L)[:, :cur]
        logits = logits_fn(prev).float()
        V = logits.shape[1]
        lp = torch.log_softmax(logits, dim=-1)
        s = process(lp, prev, repetition_penalty, False, no_repeat_ngram_size=no_repeat_ngram_size,
                    ban_ids=min_length_ban_ids(cur, eos, min_new, suppress)).float()
        acc = (s.view(B, nb, V) + st["running_beam_scores"][:, :, None]).view(B, nb * V)
        idx = top_stable(acc, 2 * nb)
        st, _, _, hits_all = beam_step(st, torch.gather(acc, 1, idx), idx, V, cur, L, eos, length_penalty,
                                       early_stopping)
        cur += 1
        if cur >= L:
            break
        if cur % eos_check == 0:
            go_on = bool(st["unsat"].any()) and not bool(hits_all.all())
            if early_stopping is True and bool(st["is_sent_finished"].all()):
                go_on = False
            if not go_on:
                break
    return st["sequences"], st["beam_scores"], st["gen_len"]
