#!/usr/bin/env python3
"""Record tests/golden/caption_metrics.npz: what the reference's metric code gives for captions made of token ids.

    python tools/make_eval_golden.py --reference <checkout of A-SHOJAEI/preference-guided-image-captioning-alignment>

Run by hand where the reference is checked out (it is not needed to run the tests).  The reference's
``evaluation/metrics.py`` is loaded as it is; a ``CaptioningMetrics`` is made with ``object.__new__`` (its ``__init__``
loads models and metric packages) and given ``_nltk = SimpleNamespace(word_tokenize=str.split)`` and a logger.  A
caption is written as its ids in decimal, joined by spaces, so ``str.split`` gives one word per id.  Called:
``_compute_cider`` (sigma 6), ``compute_diversity_metrics`` and ``compute_preference_metrics`` (preferred = the first
reference, rejected = a caption drawn for the purpose).

Corpora: every (N, K) of N in 1..8 (cycled) x K in 1..4 x vocabulary 3, 6, 40 and then some, lengths 0..13 drawn
uniformly; corpora 0..3 are forced to hold N = 1, an empty prediction, an empty reference and predictions shorter than
four ids.  No draw is rejected.  Recorded per corpus (arrays only, zero padded; a reference slot k >= K has length -1):
N, K, vocab, pred_ids [8, 13], pred_len [8], ref_ids [8, 4, 13], ref_len [8, 4], rej_ids [8, 13], rej_len [8],
cider, diversity [3] (diversity_1, diversity_2, unique_caption_ratio), preference [4] (win rate, mean preferred
similarity, mean rejected similarity, margin).
"""
import argparse
import importlib.util
import logging
import os
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NMAX, KMAX, LMAX = 8, 4, 13


def reference_metrics(reference: str):
    path = os.path.join(reference, "src", "preference_guided_image_captioning_alignment", "evaluation", "metrics.py")
    spec = importlib.util.spec_from_file_location("reference_metrics", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    me = object.__new__(mod.CaptioningMetrics)
    me._nltk = types.SimpleNamespace(word_tokenize=str.split)
    me.logger = logging.getLogger("golden")
    return me


def text(ids):
    return " ".join(str(int(t)) for t in ids)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("PGCA_REFERENCE"), required="PGCA_REFERENCE" not in os.environ)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "caption_metrics.npz"))
    ap.add_argument("--corpora", type=int, default=60)
    args = ap.parse_args()
    me = reference_metrics(args.reference)
    rng = np.random.default_rng(20261)
    C = args.corpora
    out = dict(N=np.zeros(C, np.int32), K=np.zeros(C, np.int32), vocab=np.zeros(C, np.int32),
               pred_ids=np.zeros((C, NMAX, LMAX), np.int64), pred_len=np.zeros((C, NMAX), np.int32),
               ref_ids=np.zeros((C, NMAX, KMAX, LMAX), np.int64), ref_len=np.full((C, NMAX, KMAX), -1, np.int32),
               rej_ids=np.zeros((C, NMAX, LMAX), np.int64), rej_len=np.zeros((C, NMAX), np.int32),
               cider=np.zeros(C, np.float64), diversity=np.zeros((C, 3), np.float64),
               preference=np.zeros((C, 4), np.float64))
    for c in range(C):
        N, K, vocab = 1 + (c * 3) % NMAX, 1 + c % KMAX, (3, 6, 40)[(c // KMAX) % 3]
        if c == 0:
            N = 1
        plen = rng.integers(0, LMAX + 1, N)
        rlen = rng.integers(0, LMAX + 1, (N, K))
        jlen = rng.integers(0, LMAX + 1, N)
        if c == 1:
            plen[0] = 0
        if c == 2:
            rlen[0, 0] = 0
        if c == 3:
            plen[:] = rng.integers(0, 4, N)
        out["N"][c], out["K"][c], out["vocab"][c] = N, K, vocab
        preds, refs, rejected = [], [], []
        for i in range(N):
            p, j = rng.integers(0, vocab, plen[i]), rng.integers(0, vocab, jlen[i])
            out["pred_ids"][c, i, :plen[i]], out["pred_len"][c, i] = p, plen[i]
            out["rej_ids"][c, i, :jlen[i]], out["rej_len"][c, i] = j, jlen[i]
            preds.append(text(p))
            rejected.append(text(j))
            refs.append([])
            for k in range(K):
                r = rng.integers(0, vocab, rlen[i, k])
                out["ref_ids"][c, i, k, :rlen[i, k]], out["ref_len"][c, i, k] = r, rlen[i, k]
                refs[-1].append(text(r))
        out["cider"][c] = me._compute_cider(preds, refs, 6.0)
        d = me.compute_diversity_metrics(preds)
        out["diversity"][c] = d["diversity_1"], d["diversity_2"], d["unique_caption_ratio"]
        p = me.compute_preference_metrics(preds, [r[0] for r in refs], rejected, [float(i) for i in range(N)])
        out["preference"][c] = (p["preference_win_rate"], p["avg_preferred_similarity"], p["avg_rejected_similarity"],
                                p["preference_margin"])
    assert np.isfinite(out["cider"]).all()
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {C} corpora, {int(out['N'].sum())} images, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
