"""Plain-Python restatements of ROUGE-1 / ROUGE-2 / ROUGE-L and METEOR over lists of token ids (the reference's
evaluation/metrics.py:275-338 with an id in the place of a word; stemming, lower-casing and WordNet are the identity on
ids): what ``pgca_rouge_stats``, ``pgca_meteor_stats`` and the host formulas of ``pgca_amd.evaluation`` are checked
against.  Written for clarity: the LCS is the full table, the METEOR matching pops lists as nltk's ``_match_enums`` does.

A caption is a list of ints; the references of an image are a list of such lists in which ``None`` marks an absent
reference (the kernels' len -1) and ``[]`` a present, empty one.
"""
ALPHA, BETA, GAMMA = 0.9, 3.0, 0.5      # HF ``meteor``'s defaults


def ngram_counts(tokens, n):
    out = {}
    for i in range(len(tokens) - n + 1):
        g = tuple(tokens[i:i + n])
        out[g] = out.get(g, 0) + 1
    return out


def overlap(pred, ref, n):
    """Sum over the distinct n-grams of the reference of min(count in the prediction, count in the reference)."""
    pc, rc = ngram_counts(pred, n), ngram_counts(ref, n)
    return sum(min(pc.get(g, 0), c) for g, c in rc.items())


def lcs(a, b):
    """Length of the longest common subsequence, by the whole (len(a) + 1) x (len(b) + 1) table."""
    table = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            if a[i - 1] == b[j - 1]:
                table[i][j] = table[i - 1][j - 1] + 1
            else:
                table[i][j] = max(table[i - 1][j], table[i][j - 1])
    return table[len(a)][len(b)]


def first_present(refs):
    """(k, reference k) of the lowest k whose reference is present, or (-1, None)."""
    for k, r in enumerate(refs):
        if r is not None:
            return k, r
    return -1, None


def rouge_stats(pred, refs):
    """The six integers of one image: overlap_1, overlap_2, lcs, prediction length, reference length, k used."""
    k, ref = first_present(refs)
    if k < 0:
        return [0, 0, 0, 0, 0, -1]
    return [overlap(pred, ref, 1), overlap(pred, ref, 2), lcs(pred, ref), len(pred), len(ref), k]


def f_measure(p, r):
    return 2.0 * p * r / (p + r) if p + r > 0 else 0.0


def rouge_n(pred, ref, n):
    """F of ROUGE-n."""
    o = overlap(pred, ref, n)
    return f_measure(o / max(len(pred) - n + 1, 1), o / max(len(ref) - n + 1, 1))


def rouge_l(pred, ref):
    if not pred or not ref:
        return 0.0
    length = lcs(pred, ref)
    return f_measure(length / len(pred), length / len(ref))


def rouge(preds, all_refs):
    """Mean F over ALL images of the prediction against the image's first present reference (0 for an image with
    none)."""
    total = {"rouge1": 0.0, "rouge2": 0.0, "rougeL": 0.0}
    for pred, refs in zip(preds, all_refs):
        k, ref = first_present(refs)
        if k < 0:
            continue
        total["rouge1"] += rouge_n(pred, ref, 1)
        total["rouge2"] += rouge_n(pred, ref, 2)
        total["rougeL"] += rouge_l(pred, ref)
    return {name: v / len(preds) for name, v in total.items()}


def meteor_matches(hyp, ref):
    """nltk's ``_match_enums``: the hypothesis from its last position to its first, each against the reference from its
    last remaining position to its first; a matched pair leaves both lists.  Returns the (i, j) pairs sorted by i."""
    hyp_left, ref_left = list(enumerate(hyp)), list(enumerate(ref))
    matches = []
    for i in range(len(hyp_left))[::-1]:
        for j in range(len(ref_left))[::-1]:
            if hyp_left[i][1] == ref_left[j][1]:
                matches.append((hyp_left[i][0], ref_left[j][0]))
                hyp_left.pop(i)
                ref_left.pop(j)
                break
    return sorted(matches)


def count_chunks(matches):
    """nltk's ``_count_chunks``: runs of matches adjacent in both captions."""
    if not matches:
        return 0
    chunks = 1
    for prev, cur in zip(matches, matches[1:]):
        if cur[0] == prev[0] + 1 and cur[1] == prev[1] + 1:
            continue
        chunks += 1
    return chunks


def meteor_stats(pred, refs):
    """[m, chunks] per reference, [-1, -1] for an absent one."""
    out = []
    for ref in refs:
        if ref is None:
            out.append([-1, -1])
        else:
            matches = meteor_matches(pred, ref)
            out.append([len(matches), count_chunks(matches)])
    return out


def meteor_single(pred, ref):
    if not pred or not ref:
        return 0.0
    matches = meteor_matches(pred, ref)
    m = len(matches)
    if m == 0:
        return 0.0
    precision, recall = m / len(pred), m / len(ref)
    fmean = precision * recall / (ALPHA * precision + (1.0 - ALPHA) * recall)
    penalty = GAMMA * (count_chunks(matches) / m) ** BETA
    return (1.0 - penalty) * fmean


def meteor_image(pred, refs):
    """The best score over the present references (0 when there is none)."""
    return max((meteor_single(pred, r) for r in refs if r is not None), default=0.0)


def meteor(preds, all_refs):
    return sum(meteor_image(p, r) for p, r in zip(preds, all_refs)) / len(preds)
