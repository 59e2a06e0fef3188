"""Plain-Python restatements of the caption metrics over lists of token ids (the reference's evaluation/metrics.py with
an id in the place of a word): what ``csrc/eval.hip`` and ``pgca_amd.evaluation`` are checked against.

A caption is a list of ints; the references of an image are a list of such lists in which ``None`` marks an absent
reference (the kernels' len -1) and ``[]`` a present, empty one.
"""
import math


def ngrams(tokens, n):
    return [tuple(tokens[i:i + n]) for i in range(len(tokens) - n + 1)]


def counts(tokens, n):
    out = {}
    for g in ngrams(tokens, n):
        out[g] = out.get(g, 0) + 1
    return out


def present(refs):
    return [r for r in refs if r is not None]


def key(gram):
    """The int64 key of an n-gram: 16 bits per id, the first most significant, read as a signed number."""
    k = 0
    for t in gram:
        k = (k << 16) | (int(t) & 0xffff)
    return k - (1 << 64) if k >= (1 << 63) else k


def ngram_keys(groups, lens, n, S, distinct):
    """``groups`` [G][K][S] ids, ``lens`` [G][K] (-1 absent) -> keys [G][K][S] as pgca_ngram_keys writes them."""
    out = []
    for rows, ls in zip(groups, lens):
        seen, g_out = set(), []
        for row, l in zip(rows, ls):
            l = max(0, min(int(l), S))
            r_out = []
            for t in range(S):
                k = key(row[t:t + n]) if t + n <= l else -1
                if distinct and k != -1:
                    if k in seen:
                        k = -1
                    else:
                        seen.add(k)
                r_out.append(k)
            g_out.append(r_out)
        out.append(g_out)
    return out


def doc_freq(all_refs):
    """metrics.py:489-501: every n-gram (orders 1..4) once per image."""
    df = {}
    for refs in all_refs:
        seen = set()
        for ref in present(refs):
            for n in range(1, 5):
                for g in counts(ref, n):
                    if g not in seen:
                        df[g] = df.get(g, 0) + 1
                        seen.add(g)
    return df


def cider_rows(preds, all_refs, sigma=6.0, df=None, n_docs=None):
    """metrics.py:507-570 per image, before the x10 and the mean.  Returns (scores, flags): an image with no present
    reference scores 0 with flag 1.  ``df`` / ``n_docs``: those of a larger corpus the images belong to."""
    df = doc_freq(all_refs) if df is None else df
    n_docs = len(all_refs) if n_docs is None else n_docs
    scores, flags = [], []
    for pred, refs in zip(preds, all_refs):
        refs = present(refs)
        if not refs:
            scores.append(0.0)
            flags.append(1)
            continue
        score = 0.0
        for n in range(1, 5):
            pc = counts(pred, n)
            rc = {}
            for ref in refs:
                for g, c in counts(ref, n).items():
                    rc[g] = rc.get(g, 0.0) + c / len(refs)
            num = pn = rn = 0.0
            for g in sorted(set(pc) | set(rc)):
                idf = math.log(n_docs / (df.get(g, 1) + 1e-8))
                pw, rw = pc.get(g, 0) * idf, rc.get(g, 0) * idf
                num += pw * rw
                pn += pw ** 2
                rn += rw ** 2
            score += num / math.sqrt(pn * rn) if pn > 0 and rn > 0 else 0.0
        score /= 4.0
        avg = sum(len(r) for r in refs) / len(refs)
        score *= math.exp(-(len(pred) - avg) ** 2 / (2 * sigma ** 2)) if avg > 0 else 0.0
        scores.append(score)
        flags.append(0)
    return scores, flags


def cider(preds, all_refs, sigma=6.0):
    scores, _ = cider_rows(preds, all_refs, sigma)
    return sum(scores) / len(scores) * 10.0


def bleu_stats(pred, refs):
    """The ten integers of one image: clipped matches 1..4, possible matches 1..4, prediction length, shortest present
    reference (0 when there is none)."""
    refs = present(refs)
    matches, possible = [], []
    for n in range(1, 5):
        most = {}
        for ref in refs:
            for g, c in counts(ref, n).items():
                most[g] = max(most.get(g, 0), c)
        matches.append(sum(min(c, most.get(g, 0)) for g, c in counts(pred, n).items()))
        possible.append(max(0, len(pred) - n + 1))
    return matches + possible + [len(pred), min((len(r) for r in refs), default=0)]


def bleu(stats, order):
    """Corpus BLEU of ``order`` from the ten integers summed over the images: geometric mean of the precisions 1..order
    (0 if one is 0), times the brevity penalty; no smoothing; 0 when either length is 0."""
    pred_len, ref_len = stats[8], stats[9]
    if pred_len == 0 or ref_len == 0:
        return 0.0
    prec = [stats[m] / stats[4 + m] if stats[4 + m] > 0 else 0.0 for m in range(order)]
    if min(prec) <= 0.0:
        return 0.0
    geo = math.exp(sum(math.log(p) for p in prec) / order)
    return geo * (1.0 if pred_len / ref_len > 1.0 else math.exp(1.0 - ref_len / pred_len))


def corpus_bleu(preds, all_refs):
    total = [0] * 10
    for pred, refs in zip(preds, all_refs):
        total = [a + b for a, b in zip(total, bleu_stats(pred, refs))]
    return {f"bleu_{n}": bleu(total, n) for n in range(1, 5)}


def overlap(a, b):
    """|set(a) & set(b)|, |set(a) | set(b)|."""
    return len(set(a) & set(b)), len(set(a) | set(b))


def similarity(a, b):
    """metrics.py:638-661."""
    if not a or not b:
        return 0.0
    inter, union = overlap(a, b)
    return inter / union if union > 0 else 0.0


def preference(preds, preferred, rejected):
    """metrics.py:594-625 without the correlation."""
    ps = [similarity(o, p) for o, p in zip(preds, preferred)]
    rs = [similarity(o, r) for o, r in zip(preds, rejected)]
    n = len(ps)
    return {"preference_win_rate": sum(1 for p, r in zip(ps, rs) if p > r) / n if n else 0.0,
            "avg_preferred_similarity": sum(ps) / n, "avg_rejected_similarity": sum(rs) / n,
            "preference_margin": sum(ps) / n - sum(rs) / n}


def diversity(preds):
    """metrics.py:676-708; a caption is its id list."""
    out = {}
    for n in (1, 2):
        grams = [g for p in preds for g in ngrams(p, n)]
        out[f"diversity_{n}"] = len(set(grams)) / len(grams) if grams else 0.0
    out["unique_caption_ratio"] = len({tuple(p) for p in preds}) / len(preds) if preds else 0.0
    return out
