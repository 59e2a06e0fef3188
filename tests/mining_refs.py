"""Plain numpy restatements of the preference-mining kernels (csrc/mine.hip): the id conversion, the grouped cosine
in float64 and the pairing rule of the reference's ``UltraFeedbackDataset._process_scored_captions``
(data/loader.py:416-451) with the de-duplication and ``min_tokens`` filter this project adds in front of it."""
import numpy as np

RULES = ("adjacent", "best_worst")


def candidate_rows(cand, lengths, S, base_vocab, dec_vocab, dec_pad, text_pad):
    """cand int64 [R, ld], lengths int64 [R] -> dict of dec_ids, dec_mask, text_ids (int64 [R, S]), text_mask (int32
    [R, S]), text_len, out_len (int32 [R])."""
    cand, lengths = np.asarray(cand, np.int64), np.asarray(lengths, np.int64)
    R, ld = cand.shape
    out = dict(dec_ids=np.full((R, S), dec_pad, np.int64), dec_mask=np.zeros((R, S), np.int64),
               text_ids=np.full((R, S), text_pad, np.int64), text_mask=np.zeros((R, S), np.int32),
               text_len=np.zeros(R, np.int32), out_len=np.zeros(R, np.int32))
    for r in range(R):
        n = int(min(max(int(lengths[r]), 0), ld, S))
        live = [int(v) for v in cand[r, :n]]
        if any(v < 0 or v >= dec_vocab for v in live):
            out["text_len"][r] = -1
            continue
        out["dec_ids"][r, :n] = live
        out["dec_mask"][r, :n] = 1
        text = [v for v in live if v < base_vocab]
        out["text_ids"][r, :len(text)] = text
        out["text_mask"][r, :len(text)] = 1
        out["text_len"][r], out["out_len"][r] = len(text), n
    return out


def group_cosine(img, txt, n):
    """float64 cosine of image b with its n captions: F.normalize (eps 1e-12) on both sides, then the dot product."""
    img, txt = np.asarray(img, np.float64), np.asarray(txt, np.float64)
    a = img / np.maximum(np.linalg.norm(img, axis=1, keepdims=True), 1e-12)
    t = txt / np.maximum(np.linalg.norm(txt, axis=1, keepdims=True), 1e-12)
    return (np.repeat(a, n, axis=0) * t).sum(axis=1)


def left_out(scores, dec_ids, out_len, ok, min_tokens):
    """Boolean [n] for one image: which candidates the pairing never sees."""
    n = len(scores)
    drop = np.zeros(n, bool)
    for j in range(n):
        dup = any(out_len[i] == out_len[j] and np.array_equal(dec_ids[i, :out_len[i]], dec_ids[j, :out_len[j]])
                  for i in range(j))
        drop[j] = (not np.isfinite(scores[j])) or (ok is not None and not ok[j]) or out_len[j] < min_tokens or dup
    return drop


def pair_image(scores, threshold, rule="adjacent", drop=None):
    """One image: float32 scores [n] -> (rank int32 [n], winners, losers, margins).  The sort is the reference's own
    (``list.sort(key=score, reverse=True)``, stable); the subtraction and the comparison are float32."""
    s = np.asarray(scores, np.float32)
    n = len(s)
    drop = np.zeros(n, bool) if drop is None else drop
    order = [j for j in range(n) if not drop[j]]
    order.sort(key=lambda j: float(s[j]), reverse=True)
    rank = np.full(n, -1, np.int32)
    for k, j in enumerate(order):
        rank[j] = k
    steps = range(len(order) - 1) if rule == "adjacent" else ([0] if len(order) >= 2 else [])
    win, lose, margin = [], [], []
    for k in steps:
        w, l = order[k], order[k + 1 if rule == "adjacent" else -1]
        d = np.float32(s[w] - s[l])
        if d >= np.float32(threshold):
            win.append(w), lose.append(l), margin.append(d)
    return rank, win, lose, margin


def mine_pairs(scores, dec_ids, out_len, ok, min_tokens, rule, threshold):
    """scores [B, n]; dec_ids [B*n, S]; out_len [B*n]; ok [B, n] or None -> rank [B, n], pair_win / pair_lose int32 and
    pair_margin float32 [B, n] (unused slots -1, -1, 0), pair_count int32 [B]."""
    scores = np.asarray(scores, np.float32)
    B, n = scores.shape
    ids, lens = np.asarray(dec_ids).reshape(B, n, -1), np.asarray(out_len).reshape(B, n)
    rank = np.zeros((B, n), np.int32)
    pw, pl = np.full((B, n), -1, np.int32), np.full((B, n), -1, np.int32)
    pm, cnt = np.zeros((B, n), np.float32), np.zeros(B, np.int32)
    for b in range(B):
        drop = left_out(scores[b], ids[b], lens[b], None if ok is None else np.asarray(ok)[b], min_tokens)
        rank[b], w, l, m = pair_image(scores[b], threshold, rule, drop)
        cnt[b] = len(w)
        pw[b, :len(w)], pl[b, :len(w)], pm[b, :len(w)] = w, l, m
    return rank, pw, pl, pm, cnt


def pair_rows(pw, pl, pm, cnt, dec_ids, dec_mask, cap, dec_pad):
    """The Stage-2 batch: pairs in image order, then pad rows up to ``cap``."""
    B, n = pw.shape
    S = dec_ids.shape[1]
    out = dict(preferred_ids=np.full((cap, S), dec_pad, np.int64), preferred_mask=np.zeros((cap, S), np.int64),
               rejected_ids=np.full((cap, S), dec_pad, np.int64), rejected_mask=np.zeros((cap, S), np.int64),
               pair_image=np.full(cap, -1, np.int32), preference_score=np.zeros(cap, np.float32))
    r = 0
    for b in range(B):
        for p in range(int(cnt[b])):
            w, l = b * n + pw[b, p], b * n + pl[b, p]
            out["preferred_ids"][r], out["preferred_mask"][r] = dec_ids[w], dec_mask[w]
            out["rejected_ids"][r], out["rejected_mask"][r] = dec_ids[l], dec_mask[l]
            out["pair_image"][r], out["preference_score"][r] = b, pm[b, p]
            r += 1
    out["n_pairs"] = r
    return out
